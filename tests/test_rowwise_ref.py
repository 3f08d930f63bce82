"""Host checks of tests/rowwise_ref.py (no GPU): the exact forms against torch in float64, the hand-written backward formulas against
autograd, the model's deviation non-zero and finite on the case grid, the summation rule (left to right in f32) against an emulation
of the kernels' order, the bf16 element gate against truncation, and the label reference on hand-made arrays."""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from tests import rowwise_ref as R

F64, F32 = torch.float64, torch.float32


def close(a, b, tol=1e-12):
    a, b = torch.as_tensor(a, dtype=F64), torch.as_tensor(b, dtype=F64)
    assert a.shape == b.shape
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), float((a - b).abs().max())


# ----------------------------------------------------------------------------- exact == torch, formulas == autograd
def test_lsum_is_left_to_right_in_f32():
    x = torch.randn(3, 1000, generator=torch.Generator().manual_seed(0)) * 100
    acc = np.zeros(3, dtype=np.float32)
    for j in range(1000):
        acc = (acc + x[:, j].numpy()).astype(np.float32)
    assert np.array_equal(R.lsum(x).numpy(), acc)
    assert np.array_equal(R.lsum(x.t().contiguous(), 0).numpy(), acc)
    assert not np.array_equal(acc, x.double().sum(-1).float().numpy())       # (the order is visible at this length)


@pytest.mark.parametrize("H", [4, 260, 1028])
def test_layernorm_exact_is_torch(H):
    c = R.ln_case(H, 9, False, True)
    ref = Fn.layer_norm(c.x.double(), (H,), c.w.double(), c.b.double(), R.f32v(c.eps)) * c.rs.double()[:, None]
    close(c.exact["y"], ref)


@pytest.mark.parametrize("with_kr,res_rows", [(False, 0), (True, 0), (True, 7)])
def test_layernorm_res_and_backward_are_autograd(with_kr, res_rows):
    H, M = 260, 70
    c = R.lnres_case(H, M, with_kr, res_rows, 1e-5)
    u = c.fx["u"].clone().requires_grad_(True)
    g, b = c.gamma.double().requires_grad_(True), c.beta.double().requires_grad_(True)
    y = Fn.layer_norm(u, (H,), g, b, R.f32v(1e-5))
    close(c.fx["y"], y.detach())
    through = R.layernorm_res(c.z, c.keep, c.res, res_rows, c.gamma, c.beta, 1e-5, leaf=u.detach())
    close(through["y"], y.detach())
    (y * c.dy.double()).sum().backward()
    bw = R.layernorm_bwd(c.dy, c.fx["xhat"], c.fx["rstd"], c.gamma, c.keep, c.dg0, c.db0)
    close(bw["du"], u.grad)
    close(bw["dz"], u.grad * (c.keep.double() if with_kr else 1.0))         # d/dz of u = z * keep + res
    close(bw["dgamma"], g.grad + c.dg0.double())
    close(bw["dbeta"], b.grad + c.db0.double())


@pytest.mark.parametrize("gelu", [False, True])
def test_rmsnorm_and_backward_are_autograd(gelu):
    H, M = 260, 9
    I = R.rms_bwd_inputs(H, M)
    x, w = I.x.double().requires_grad_(True), I.w.double().requires_grad_(True)
    rstd = torch.rsqrt((x * x).mean(-1) + R.f32v(R.RMS_EPS))
    y = x * rstd[:, None] * w
    y = Fn.gelu(y) if gelu else y
    f = R.rmsnorm_fwd(I.x, I.w, R.RMS_EPS, gelu)
    close(f["y"], y.detach()); close(f["rstd"], rstd.detach())
    (y * I.dy.double()).sum().backward()
    bw = R.rmsnorm_bwd(I.dy, I.x, rstd.detach(), I.w, I.dres, gelu, I.dw0)
    close(bw["dx"], x.grad + I.dres.double())
    close(bw["dw"], w.grad + I.dw0.double())
    if not gelu:
        close(R.rmsnorm_dw(I.dy, I.x, rstd.detach(), I.dw0)["dw"], w.grad + I.dw0.double())


def test_cross_entropy_exact_is_torch():
    V, ldl, n, scale = 1003, 1024, 37, 0.37
    z = R.ce_logits(50, V, ldl, "normal3", False)
    rows = [(7 * i + 3) % 50 for i in range(n)]
    t = R.ce_targets(n, V, ldl)
    out = R.cross_entropy(z, rows, t, V, scale, ldl + 8)
    zz = z[rows][:, :V].double().requires_grad_(True)
    tt = torch.tensor([v if 0 <= v < V else -100 for v in t])
    loss = Fn.cross_entropy(zz, tt, ignore_index=-100, reduction="sum") * R.f32v(scale)
    loss.backward()
    close(out["loss"], loss.detach())
    close(out["dlogits"][:, :V], zz.grad)
    assert not out["dlogits"][:, V:].any() and not out["dlogits"][~out["valid"]].any() and not out["nll"][~out["valid"]].any()
    close(out["nll"], Fn.cross_entropy(zz.detach(), tt, ignore_index=-100, reduction="none"))


@pytest.mark.parametrize("clip", R.CASES["adamw"]["clip"])
@pytest.mark.parametrize("denom", R.CASES["adamw"]["denom"])
def test_adamw_exact_is_torch(clip, denom):
    n, wd, hp = 1000, 0.1, {k: R.f32v(v) for k, v in R.ADAM.items()}
    g = torch.Generator().manual_seed(3)
    p0 = torch.randn(n, generator=g)
    gs = 0.5
    p = p0.double().clone().requires_grad_(True)
    opt = torch.optim.AdamW([p], lr=hp["lr"], betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"], weight_decay=R.f32v(wd))
    pe, me, ve = p0, torch.zeros(n), torch.zeros(n)
    for step in (1, 2, 3):
        gr = torch.randn(n, generator=g) * (3.0 if clip == "active" else 0.01)
        sq, max_norm = (None, 1.0) if clip == "none" else (R.sqnorm(gr), 0.0 if clip == "max_norm0" else 1.0)
        eff = R.f32v(gs) / (max(R.f32v(denom), 1.0) if denom is not None else 1.0)
        p.grad = gr.double() * eff
        if clip in ("inactive", "active"):
            norm = torch.nn.utils.clip_grad_norm_([p], 1.0)
            assert (norm > 1.0) == (clip == "active")
        opt.step()
        pe, me, ve = R.adamw(pe, gr, me, ve, wd=wd, step=step, sq=sq, max_norm=max_norm, grad_scale=gs, denom=denom, **R.ADAM)
        close(pe, p.detach(), 1e-11)
    close(R.sqnorm(gr, 2.5), (gr.double() ** 2).sum() + 2.5)


# ----------------------------------------------------------------------------- the model deviates, finitely; exactly-defined outputs do not
def deviates(exact, model, width, what):
    m = R.row_errors(model, exact, width)
    assert torch.isfinite(m).all() and float(m.max()) > 0, what


@pytest.mark.parametrize("H", R.HS_FWD)
def test_model_deviation_forward_norms(H):
    for M in (1, 3, 9, 37):
        for bf in (False, True):
            for rs in (False, True):
                c = R.ln_case(H, M, bf, rs)
                deviates(c.exact["y"], c.model["y"], H, ("ln f32", H, M, bf, rs))
                deviates(c.exact["y"], R.rb(c.model["y"]), H, ("ln bf16", H, M, bf, rs))
                if rs:
                    z = c.rs == 0
                    assert not c.exact["y"][z].any() and not c.model["y"][z].any()
    for M in (1, 7, 9, 37):
        for bf, gelu in ((False, False), (False, True), (True, False)):
            c = R.rms_case(H, M, bf, gelu)
            deviates(c.exact["y"], c.model["y"], H, ("rms", H, M, bf, gelu))
            deviates(c.exact["rstd"], c.model["rstd"], M, ("rms rstd", H, M))
            if M > 1:                                                         # the zero row: exactly 0 in both forms
                assert not c.exact["y"][0].any() and not c.model["y"][0].any()


@pytest.mark.parametrize("H", R.HS_BWD)
def test_model_deviation_rmsnorm_backward(H):
    for M in (1, 9, 37):
        I = R.rms_bwd_inputs(H, M)
        for xb, dyb, gelu in ((False, False, False), (False, False, True), (True, True, False), (False, True, False)):
            x, dy = (I.x.to(R.BF16) if xb else I.x), (I.dy.to(R.BF16) if dyb else I.dy)
            r = R.rstd_of(x)
            e, m = R.rmsnorm_bwd(dy, x, r, I.w, I.dres, gelu, I.dw0), R.rmsnorm_bwd(dy, x, r, I.w, I.dres, gelu, I.dw0, model=True)
            deviates(e["dx"], m["dx"], H, ("dx", H, M))
            deviates(e["dw"], m["dw"], H, ("dw", H, M))
        z = torch.zeros_like(I.dy)
        assert torch.equal(R.rmsnorm_bwd(z, I.x, r, I.w, None, False, I.dw0, model=True)["dw"], I.dw0.double())
        assert torch.equal(R.rmsnorm_dw(z, I.x, r, I.dw0, model=True)["dw"], I.dw0.double())


@pytest.mark.parametrize("H", R.HS_LNRES)
def test_model_deviation_layernorm_res(H):
    for M, rr in ((1, 0), (33, 0), (70, 7)):
        for kr in (False, True):
            for eps in (1e-5, 1e-12):
                c = R.lnres_case(H, M, kr, rr if kr else 0, eps)
                for k in ("xhat", "y"):
                    deviates(c.fx[k], c.fm[k], H, (k, H, M, kr, eps))
                deviates(c.fx["rstd"], c.fm["rstd"], M, ("rstd", H, M))
                for k in ("du", "dz"):
                    deviates(c.bx[k], c.bm[k], H, (k, H, M, kr, eps))
                for k in ("dgamma", "dbeta"):
                    deviates(c.bx[k], c.bm[k], H, (k, H, M, kr, eps))


def test_model_deviation_cross_entropy_and_optimizer():
    for V, ldl in R.CASES["cross_entropy"]["V_ldl"]:
        for bf in (False, True):
            z, t = R.ce_logits(37, V, ldl, "normal3", bf), R.ce_targets(37, V, ldl)
            e, m = R.cross_entropy(z, None, t, V, 0.37, ldl), R.cross_entropy(z, None, t, V, 0.37, ldl, model=True)
            deviates(e["nll"], m["nll"], 37, ("nll", V))
            deviates(e["dlogits"], R.rb(m["dlogits"]), ldl, ("dlogits", V))
            assert float(m["loss"]) != float(e["loss"]) and np.isfinite(float(m["loss"]))
            inv = ~e["valid"]
            assert inv.sum() >= 2 and not m["dlogits"][inv].any() and not m["dlogits"][:, V:].any() and not m["nll"][inv].any()
    g = torch.randn(10007, generator=torch.Generator().manual_seed(1))
    assert float(R.sqnorm(g, model=True)) != float(R.sqnorm(g))
    z = torch.zeros(10007)
    for e, m in zip(R.adamw(g, g, z, z, wd=0.1, step=1, **R.ADAM), R.adamw(g, g, z, z, wd=0.1, step=1, model=True, **R.ADAM)):
        pad = lambda t: torch.cat([t, torch.zeros(1024 * 10 - 10007, dtype=F64)])
        deviates(pad(e), pad(m), 1024, "adamw")


# ----------------------------------------------------------------------------- left to right in f32 dominates the kernels' order
def kernel_order_sum(x, lanes=64):
    """The kernels' row sum in f32: lane l adds the float4 chunks l, l + lanes, ... (each as ((a + b) + c) + d), then an xor tree."""
    M, H = x.shape
    nv = H // 4
    I = -(-nv // lanes)
    q = torch.zeros(M, I * lanes, 4)
    q[:, :nv] = x.reshape(M, nv, 4)
    q = ((q[..., 0] + q[..., 1]) + q[..., 2]) + q[..., 3]
    q = q.reshape(M, I, lanes)
    s = torch.zeros(M, lanes)
    for i in range(I):
        s = s + q[:, i]
    o = lanes // 2
    while o:
        s = s + s[:, torch.arange(lanes) ^ o]
        o //= 2
    return s[:, 0]


def rsqrt_1ulp(x):
    """An rsqrt that is within 1 ulp of the exact value but never correctly rounded: the f32 neighbour on the other side of it."""
    ex = torch.rsqrt(x.double())
    cr = ex.float()
    step = torch.where(cr.double() >= ex, torch.tensor(-1, dtype=torch.int32), torch.tensor(1, dtype=torch.int32))
    return (cr.view(torch.int32) + step).view(F32)


@pytest.mark.parametrize("H", (4, 128, 252, 256, 260, 1028, 2048, 5120))
def test_left_to_right_dominates_the_kernel_order_norms(H):
    for M in (9, 37):
        c = R.ln_case(H, M, False, False)
        x = c.x
        d = x - (kernel_order_sum(x) / H)[:, None]
        rstd = rsqrt_1ulp(kernel_order_sum(d * d) / H + R.f32v(c.eps))
        y = d * rstd[:, None] * c.w + c.b
        e, m = R.row_errors(y, c.exact["y"], H).max(), R.row_errors(c.model["y"], c.exact["y"], H).max()
        assert float(e) <= 2 * float(m), ("ln", H, M, float(e / m))
        c = R.rms_case(H, M, False, False)
        rstd = rsqrt_1ulp(kernel_order_sum(c.x * c.x) / H + R.f32v(c.eps))
        y = c.x * rstd[:, None] * c.w
        e, m = R.row_errors(y, c.exact["y"], H).max(), R.row_errors(c.model["y"], c.exact["y"], H).max()
        assert float(e) <= 2 * float(m), ("rms", H, M, float(e / m))
        e, m = R.row_errors(rstd, c.exact["rstd"], M).max(), R.row_errors(c.model["rstd"], c.exact["rstd"], M).max()
        assert float(e) <= 2 * float(m), ("rstd", H, M, float(e / m))


@pytest.mark.parametrize("V,ldl", R.CASES["cross_entropy"]["V_ldl"])
def test_left_to_right_dominates_the_kernel_order_loss(V, ldl):
    """256 threads stride over float4 chunks, a scalar tail, an xor tree per wave, then the 4 waves in order; the exponential is a
    hardware exp2 of the f32-rounded x * log2(e), the pessimistic model of __expf."""
    z, t = R.ce_logits(37, V, ldl, "normal3", False), R.ce_targets(37, V, ldl)
    ex, mo = R.cross_entropy(z, None, t, V, 1.0, ldl), R.cross_entropy(z, None, t, V, 1.0, ldl, model=True)
    zz = z[:, :V]
    m = zz.amax(-1)
    fexp = lambda a: torch.exp2((a * 1.4426950408889634).float().double()).float()
    e = fexp(zz - m[:, None])
    nv = V // 4
    body = torch.zeros(37, max(1, -(-nv // 256)) * 1024)
    body[:, :nv * 4] = e[:, :nv * 4]
    s = kernel_order_sum(body, lanes=256) * 0 if nv == 0 else None
    q = body.reshape(37, -1, 256, 4)
    q = ((q[..., 0] + q[..., 1]) + q[..., 2]) + q[..., 3]
    th = torch.zeros(37, 256)
    for i in range(q.shape[1]):
        th = th + q[:, i]
    for j, c in enumerate(range(nv * 4, V)):
        th[:, j] = th[:, j] + e[:, c]
    th = th.reshape(37, 4, 64)
    o = 32
    while o:
        th = th + th[:, :, torch.arange(64) ^ o]
        o //= 2
    S = ((th[:, 0, 0] + th[:, 1, 0]) + th[:, 2, 0]) + th[:, 3, 0]
    lse = m + (torch.log2(S.double()).float() * 0.6931471805599453).float()     # __logf: log2 * ln 2
    nll = torch.where(ex["valid"], lse - zz.gather(1, torch.tensor(t).clamp(0, V - 1)[:, None])[:, 0], torch.zeros(()))
    assert s is None or not s.any()
    e_, m_ = R.row_errors(nll, ex["nll"], 37).max(), R.row_errors(mo["nll"], ex["nll"], 37).max()
    assert float(e_) <= 2 * float(m_), (V, float(e_ / m_))


# ----------------------------------------------------------------------------- the bf16 element gate
@pytest.mark.parametrize("H", (4, 260, 2048))
def test_elem_gate_accepts_nearest_even_and_rejects_truncation(H):
    c = R.ln_case(H, 37, False, False)
    ok, ratio, _ = R.elem_gate(R.rb(c.model["y"]), c.exact["y"], c.model["y"], H)
    assert ok and ratio <= 1.0
    ok, ratio, _ = R.elem_gate(R.trunc_bf16(c.model["y"]), c.exact["y"], c.model["y"], H)
    assert not ok and ratio > 1.0
    c = R.rms_case(H, 37, True, False)
    assert R.elem_gate(R.rb(c.model["y"]), c.exact["y"], c.model["y"], H)[0]
    assert not R.elem_gate(R.trunc_bf16(c.model["y"]), c.exact["y"], c.model["y"], H)[0]
    assert float(R.ulp_bf16(torch.tensor(1.0, dtype=F64))) == 2.0 ** -7 and float(R.ulp_bf16(torch.tensor(1.99, dtype=F64))) == 2.0 ** -7
    assert float(R.ulp_bf16(torch.tensor(-0.5, dtype=F64))) == 2.0 ** -8


def test_last_place_moves_one_f32_ulp_away_from_exact():
    e = torch.tensor([1.0, 1.0, -3.0, 0.0, 0.0], dtype=F64)
    m = torch.tensor([1.0, 1.0 - 2.0 ** -24, -3.0 - 2.0 ** -22, 0.0, 1e-30], dtype=F64)
    w = R.last_place(m, e)
    assert torch.equal(w[:4], torch.tensor([1.0 + 2.0 ** -23, 1.0 - 2.0 ** -24 - 2.0 ** -24, -3.0 - 2.0 ** -22 - 2.0 ** -22, 0.0], dtype=F64))
    assert float(w[4]) > 1e-30
    assert float(R.last_place(34.5, 34.6)) == 34.5 - 2.0 ** -18
    u = R.unordered(torch.tensor([4.0, 0.5, 0.0], dtype=F64), torch.tensor([4.0, 0.6, 0.0], dtype=F64), 16)
    assert torch.equal(u, torch.tensor([4.0 + 2 * 2.0 ** -21, 0.5 - 2 * 2.0 ** -21, 0.0], dtype=F64))


# ----------------------------------------------------------------------------- labels
def test_label_rows_on_hand_made_arrays():
    assert R.label_rows([[5]]) == ([], [], 0)
    assert R.label_rows([[-100, 7, -100, 9]]) == ([0, 2], [7, 9], 2)
    # a valid label at a row's position 0 is nobody's target; the last position of a row has none
    assert R.label_rows([[1, -100, -100], [2, 3, -100], [4, -100, 6]]) == ([3, 7], [3, 6], 2)
    assert R.label_rows([[-100, -100], [-100, -100]]) == ([], [], 0)
    for B, L in R.CASES["label_rows"]["BL"]:
        lab = R.make_labels(B, L, "all")
        rows, tg, n = R.label_rows(lab)
        assert n == B * (L - 1) and all(r % L != L - 1 for r in rows) and rows == sorted(rows)
        assert R.label_rows(R.make_labels(B, L, "none"))[2] == 0 and R.label_rows(R.make_labels(B, L, "pos0"))[2] == 0
        rows, tg, n = R.label_rows(R.make_labels(B, L, "chunk_last"))
        assert n == (1 if L > 1 else 0) and (n == 0 or rows[0] == max(p for p in range(min(B * L, 1024)) if p % L + 1 < L))

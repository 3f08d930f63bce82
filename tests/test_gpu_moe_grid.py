"""-m gpu: the shared + sparse MoE projector (csrc/moe.hip and the two grouped forms of the GEMM) against the float64 reference of
tests/moe_ref.py, row by row, over a grid of token counts, expert counts and per-expert slot counts set by construction.

Gate (tests/attention_ref.gate):  max_r e_r <= 2 max_r m_r  with  e_r = |got_r - exact_r| / (|exact_r| + rho)  and m_r the same
statistic of the reference's rounding model -- the bound is computed from the reference's two forms alone.  Rows: the tokens of y, the
rows of a weight gradient; a bias / norm gradient is one row.  aux: the scalar gate of moe_ref.gate_aux (factor 2 against the model's
deviation); exactly 0 in eval mode.  The gradients of an expert without slots must be exactly 0.  No token is excluded anywhere.
Every check prints  ``MOEGRID <path> <case> <tensor> e/m=<ratio>``; the measured table is profiles/moe_grid.md.

test_module         through MoEAudioProjector (ta_moe_pack_images, the op wrappers, ta_moe_projector_backward_dev), every case of
                    moe_ref.CASES.  The llm_dim = 196 case is forward only: the backward contracts over llm_dim and the library's GEMM
                    takes K in multiples of 64.
test_cabi_*         through the C ABI: tape / workspace pre-filled with 0xFF bytes (NaN as bf16 and f32, -1 as int) and every output
                    with 7; experts in separate, non-monotonic allocations (the per-expert launch fallback of forward and backward);
                    the host-d_aux entry point against the device one; ta_moe_router_aux_grads against the reference's aux-only share.
"""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

from tests import moe_ref as M

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tiny_audio_amd import _lib
    from tiny_audio_amd.projectors import MoEAudioProjector

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
KINDS = ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias")


def dev(t, dtype=None):
    if t is None:
        return None
    return (t.to(dtype) if dtype is not None else t).to(DEV).contiguous()


def check_all(path, r, y, aux, grads, exact=None, model=None):
    """The gates on y, aux and every parameter gradient of one run.  ``exact`` / ``model``: (forward dict, gradients) overriding the
    case's own (the aux-only share)."""
    c = r.c
    fx, gx = exact or (r.fx, r.gx)
    fm, gm = model or (r.fm, r.gm)
    if y is not None:
        y = y.detach().float().cpu().reshape(c.T, c.D)
        assert torch.isfinite(y).all()
        ok, ratio, w = M.gate(y, fx["y"], fm["y"], width=c.D)
        print(f"MOEGRID {path} {c.id} y e/m={ratio:.3f} worst=token {w}")
        assert ok, (path, c.id, "y", ratio, w)
    if aux is not None:
        aux = float(aux)
        if not c.training:
            assert aux == 0.0
        else:
            ok, ratio = M.gate_aux(aux, float(fx["aux"]), float(fm["aux"]), M.aux_f32(fm, c.E, M.COEF, M.ZCOEF))
            print(f"MOEGRID {path} {c.id} aux e/m={ratio:.3f} (got {aux:.9e}, exact {float(fx['aux']):.9e}, model {float(fm['aux']):.9e})")
            assert ok, (path, c.id, "aux", ratio)
    for n, g in (grads or {}).items():
        g = g.detach().float().cpu()
        assert torch.isfinite(g).all(), n
        if n.startswith("experts.") and c.counts[int(n.split(".")[1])] == 0:
            assert not g.any(), f"{n}: an expert without slots has a gradient of exactly 0"
            assert not gx[n].any()
            continue
        ok, ratio, w = M.gate(g, gx[n], gm[n], width=M.width_of(n, gx[n]))
        print(f"MOEGRID {path} {c.id} {n} e/m={ratio:.3f} worst=row {w}")
        assert ok, (path, c.id, n, ratio, w)


# ----------------------------------------------------------------------------- through the module
@pytest.mark.parametrize("cid", M.ALL)
def test_module(cid):
    r = M.ref(cid); c = r.c
    cfg = SimpleNamespace(encoder_dim=M.ENC, llm_dim=c.D, projector_hidden_dim=c.H, num_experts=c.E, num_experts_per_tok=2,
                          projector_pool_stride=M.K, router_aux_loss_coef=M.COEF, router_z_loss_coef=M.ZCOEF, router_jitter_noise=0.0)
    p = MoEAudioProjector(cfg).to(DEV)
    p.load_state_dict(r.I["W"])
    p.train(c.training)
    y = p(dev(r.I["x"]), jitter_noise=dev(r.I["noise"]))
    aux = p.get_aux_loss()
    assert y.shape == (c.B, c.N, c.D)
    grads = None
    if c.D % 64 == 0:
        loss = (y * dev(r.I["dy"])).sum()
        if c.training:
            loss = loss + c.d_aux * aux
        loss.backward()
        grads = {n: prm.grad for n, prm in p.named_parameters()}
        assert set(grads) == set(r.gx) and all(g is not None for g in grads.values())
    torch.cuda.synchronize()
    check_all("module", r, y, aux, grads)


# ----------------------------------------------------------------------------- through the C ABI
SCATTER = (3, 0, 5, 1, 6, 2, 8, 4, 7)       # where adapter i sits in a buffer of n + 2 slots: neither monotonic nor at a constant stride


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def slots_of(stacked, scatter, fill=None):
    """[n, ...] -> n views: the rows of ``stacked`` itself (constant stride), or copies placed at SCATTER in a larger buffer."""
    n = stacked.shape[0]
    if not scatter:
        return list(stacked.unbind(0)), stacked
    big = torch.full((n + 2,) + tuple(stacked.shape[1:]), 0.0 if fill is None else fill, device=DEV, dtype=stacked.dtype)
    views = [big[SCATTER[i]] for i in range(n)]
    if fill is None:
        for v, s in zip(views, stacked.unbind(0)):
            v.copy_(s)
    return views, big


def cabi_weights(r, scatter):
    """ta_moe_weights over images made by ta_moe_pack_images.  -> (struct, everything that must stay alive)."""
    c, L_ = r.c, _lib.lib()
    n, H, In, D = c.E + 1, c.H, M.ENC * M.K, c.D
    Wd = {k: dev(v) for k, v in r.I["W"].items()}
    ads = M.adapters(c.E)
    parr = lambda s: (C.c_void_p * n)(*[Wd[a + s].data_ptr() for a in ads])
    img = dict(w1=torch.empty((n, H, In), device=DEV, dtype=BF16), w1_t=torch.empty((n, In, H), device=DEV, dtype=BF16),
               w2=torch.empty((n, D, H), device=DEV, dtype=BF16), w2_t=torch.empty((n, H, D), device=DEV, dtype=BF16),
               b1=torch.empty((n, H), device=DEV, dtype=F32), b2=torch.empty((n, D), device=DEV, dtype=F32))
    _lib.check(L_.ta_moe_pack_images(parr("fc1.weight"), parr("fc1.bias"), parr("fc2.weight"), parr("fc2.bias"), n, H, In, D, ptr(img["w1"]),
                                     ptr(img["w1_t"]), ptr(img["w2"]), ptr(img["w2_t"]), ptr(img["b1"]), ptr(img["b2"]), stream()),
               "ta_moe_pack_images")
    wts = _lib.MoeWeights(enc_dim=M.ENC, k=M.K, hidden=H, llm_dim=D, num_experts=c.E, eps=1e-6, aux_coef=M.COEF, z_coef=M.ZCOEF,
                          norm_w=Wd["norm.weight"].data_ptr(), router_w=Wd["router.weight"].data_ptr())
    keep = [Wd, img]
    for kind, t in img.items():
        views, big = slots_of(t, scatter)
        arr = (C.c_void_p * n)(*[v.data_ptr() for v in views])
        setattr(wts, kind, C.cast(arr, C.POINTER(C.c_void_p)))
        keep += [views, big, arr]
    return wts, keep


def cabi_run(r, scatter=False, poison=False, host_d_aux=False, aux_only=False):
    """Forward + backward (or ta_moe_router_aux_grads) of one case through the C ABI.  -> (y, aux, {name: gradient})."""
    c, L_ = r.c, _lib.lib()
    n, H, In, D = c.E + 1, c.H, M.ENC * M.K, c.D
    wts, keep = cabi_weights(r, scatter)
    x, noise, dy = dev(r.I["x"]), dev(r.I["noise"]), dev(r.I["dy"])
    buf = (lambda nb: torch.full((nb,), 0xFF, device=DEV, dtype=torch.uint8)) if poison else (lambda nb: torch.empty(nb, device=DEV, dtype=torch.uint8))
    tape = buf(L_.ta_moe_tape_bytes(C.byref(wts), c.B, c.S))
    ws = buf(L_.ta_moe_bwd_workspace_bytes(C.byref(wts), c.B, c.S))
    seven = lambda *s: torch.full(s, 7.0, device=DEV, dtype=F32)
    y, aux = seven(c.T, D), seven(1)
    _lib.check(L_.ta_moe_projector_forward(C.byref(wts), ptr(x), c.B, c.S, ptr(noise), int(c.training), ptr(y), ptr(aux), ptr(tape), stream()),
               "ta_moe_projector_forward")
    g_norm, g_router = seven(In), seven(c.E, In)
    da = torch.tensor([c.d_aux], device=DEV, dtype=F32)
    if aux_only:
        _lib.check(L_.ta_moe_router_aux_grads(C.byref(wts), ptr(x), c.B, c.S, ptr(da), ptr(noise), int(c.training), ptr(tape), ptr(g_norm),
                                              ptr(g_router), ptr(ws), ws.numel(), stream()), "ta_moe_router_aux_grads")
        torch.cuda.synchronize()
        return y, aux, {"norm.weight": g_norm, "router.weight": g_router}
    outs, arrs = {}, {}
    for kind, shape in (("fc1.weight", (n, H, In)), ("fc1.bias", (n, H)), ("fc2.weight", (n, D, H)), ("fc2.bias", (n, D))):
        views, big = slots_of(seven(*shape), scatter, fill=7.0)
        outs[kind] = views
        arrs[kind] = (C.c_void_p * n)(*[v.data_ptr() for v in views])
        keep += [big]
    tail = (ptr(noise), int(c.training), ptr(tape), ptr(g_norm), ptr(g_router), arrs["fc1.weight"], arrs["fc1.bias"], arrs["fc2.weight"],
            arrs["fc2.bias"], ptr(ws), ws.numel(), stream())
    if host_d_aux:
        _lib.check(L_.ta_moe_projector_backward(C.byref(wts), ptr(x), c.B, c.S, ptr(dy), c.d_aux, *tail), "ta_moe_projector_backward")
    else:
        _lib.check(L_.ta_moe_projector_backward_dev(C.byref(wts), ptr(x), c.B, c.S, ptr(dy), ptr(da), *tail), "ta_moe_projector_backward_dev")
    torch.cuda.synchronize()
    grads = {"norm.weight": g_norm, "router.weight": g_router}
    for i, a in enumerate(M.adapters(c.E)):
        for kind in KINDS:
            grads[a + kind] = outs[kind][i]
    return y, aux, grads


# training with jitter, d_aux = 3, experts with 65 / 64 / 1 / 0 slots; 2T > 1024 with an empty expert and every count of the issue
CABI_CASES = ["T65-E4-noise", "T1100-E8-skew-train"]


@pytest.mark.parametrize("cid", CABI_CASES)
def test_cabi_poisoned_tape_and_workspace(cid):
    """The tape and the workspace need no initial contents: the padding slots of h_e, act_e, dy_slot and dh_e are never written and
    only ever masked through perm == -1, and every integer field (topi, seg, kr, perm, slot_of) is written in full before it is read."""
    r = M.ref(cid)
    check_all("cabi-poisoned", r, *cabi_run(r, poison=True))


@pytest.mark.parametrize("cid", CABI_CASES)
def test_cabi_non_strided_experts(cid):
    """Experts (weights, biases and gradient outputs) in separate, non-monotonic places: expert_stride() answers 0 and forward and
    backward take the one-launch-per-expert fallback."""
    r = M.ref(cid)
    check_all("cabi-per-expert", r, *cabi_run(r, scatter=True, poison=True, host_d_aux=True))


def test_cabi_host_d_aux_vs_dev():
    """ta_moe_projector_backward (d_aux by value) and ta_moe_projector_backward_dev (read on the device): both against the reference."""
    r = M.ref("T65-E4-zeroframes")
    check_all("cabi-host-d_aux", r, *cabi_run(r, host_d_aux=True))
    check_all("cabi-dev-d_aux", r, *cabi_run(r, host_d_aux=False))


@pytest.mark.parametrize("cid", ["T65-E4-zeroframes", "T513-E3-train"])
def test_cabi_router_aux_grads(cid):
    """ta_moe_router_aux_grads against the reference's aux-only share: the gradients of d_aux * aux alone (dy = 0)."""
    r = M.ref(cid); c = r.c
    dy0 = torch.zeros_like(r.I["dy"])
    exact = M.backward_exact(r.I["x"], r.I["W"], dy0, c.d_aux, M.K, c.E, **r.kw)
    model = M.backward_model(r.I["x"], r.I["W"], dy0, c.d_aux, M.K, c.E, rounded=True, **r.kw)
    _, _, grads = cabi_run(r, aux_only=True, poison=True)
    check_all("cabi-aux-share", r, None, None, grads, exact=exact, model=model)

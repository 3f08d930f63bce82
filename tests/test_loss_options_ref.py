"""Pins tests/loss_options_ref.py (no GPU): its float64 form against torch.nn.functional.cross_entropy(label_smoothing=) and its
autograd, against transformers' LabelSmoother, the z-loss term against autograd of zc * logsumexp^2, and eps = zc = 0 against
rowwise_ref.cross_entropy bit for bit."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import loss_options_ref as LO
from tests import rowwise_ref as R

F64 = torch.float64
V, LDL, N, SCALE = 1003, 1024, 37, 0.37


def _case(kind="normal3", bf16=False):
    z = R.ce_logits(N, V, LDL, kind, bf16)
    return z, R.ce_targets(N, V, LDL)


def _torch_inputs(z, t):
    """The valid rows as a float64 leaf, their targets."""
    tt = torch.tensor(t)
    ok = (tt >= 0) & (tt < V)
    leaf = z[:, :V].to(F64)[ok].clone().requires_grad_(True)
    return leaf, tt[ok], ok


@pytest.mark.parametrize("eps", [0.1, 0.9])
@pytest.mark.parametrize("kind", ["normal3", "shift-3000", "bf16x5"])
def test_label_smoothing_is_torch_cross_entropy(eps, kind):
    z, t = _case(kind, kind == "bf16x5")
    e = LO.cross_entropy_opt(z, None, t, V, SCALE, LDL, eps=eps)
    e32, s32 = R.f32v(eps), R.f32v(SCALE)                           # the f32 bits the C ABI carries
    leaf, tt, ok = _torch_inputs(z, t)
    ref = F.cross_entropy(leaf, tt, label_smoothing=e32, reduction="sum")
    (g,) = torch.autograd.grad(ref * s32, leaf)
    ref = ref.detach()
    assert abs(float(e["obj"].sum()) - float(ref)) <= 1e-12 * abs(float(ref))
    assert abs(float(e["loss"]) - float(ref) * s32) <= 1e-12 * abs(float(ref) * s32)
    rows = F.cross_entropy(leaf, tt, label_smoothing=e32, reduction="none").detach()
    assert float((e["obj"][ok] - rows).abs().max()) <= 1e-12 * float(rows.abs().max())
    assert float((e["dlogits"][ok][:, :V] - g).abs().max()) <= 1e-12
    # invalid targets and the padding columns: exact zeros; nll is the plain one
    assert not e["obj"][~ok].any() and not e["nll"][~ok].any() and not e["dlogits"][~ok].any() and not e["dlogits"][:, V:].any()
    plain = R.cross_entropy(z, None, t, V, SCALE, LDL)
    assert torch.equal(e["nll"], plain["nll"])


def test_label_smoothing_is_transformers_label_smoother():
    """LabelSmoother(epsilon)(outputs, labels, shift_labels=True): mean over the label tokens; it sums in float32."""
    tpu = pytest.importorskip("transformers.trainer_pt_utils")
    eps, B, L, Vs = 0.1, 3, 9, 50
    g = torch.Generator().manual_seed(5)
    logits = (torch.randn(B, L, Vs, generator=g) * 3).float()
    labels = torch.randint(0, Vs, (B, L), generator=g)
    labels[0, :4] = -100
    labels[2, 6:] = -100
    got = float(tpu.LabelSmoother(epsilon=eps)({"logits": logits}, labels, shift_labels=True))
    rows, tg, n = R.label_rows(labels.tolist())
    e = LO.cross_entropy_opt(logits.reshape(B * L, Vs), rows, tg, Vs, 1.0 / n, Vs, eps=eps)
    want = float(e["loss"])
    assert abs(got - want) <= 8 * 2.0 ** -24 * abs(want), (got, want)                      # float32 resolution of a handful of sums
    same = float(LO.objective(logits, labels, eps=R.f32v(eps), num_items=1.0 / R.f32v(1.0 / n)))    # (the f32 bits of 1 / n, as ``want``)
    assert abs(same - want) <= 1e-12 * abs(want)


@pytest.mark.parametrize("zc", [1e-4, 1e-2])
def test_z_loss_term_is_autograd_of_lse_squared(zc):
    z, t = _case()
    c32, s32 = R.f32v(zc), R.f32v(SCALE)
    e = LO.cross_entropy_opt(z, None, t, V, SCALE, LDL, zc=zc)
    p = R.cross_entropy(z, None, t, V, SCALE, LDL)
    leaf, tt, ok = _torch_inputs(z, t)
    term = c32 * torch.logsumexp(leaf, -1) ** 2
    (g,) = torch.autograd.grad(term.sum() * s32, leaf)
    term = term.detach()
    assert float(((e["obj"] - p["nll"])[ok] - term).abs().max()) <= 1e-12 * float(term.abs().max())
    assert float(((e["dlogits"] - p["dlogits"])[ok][:, :V] - g).abs().max()) <= 1e-12
    # both options at once: the sum of the two
    both = LO.cross_entropy_opt(z, None, t, V, SCALE, LDL, eps=0.1, zc=zc)
    ref = F.cross_entropy(leaf, tt, label_smoothing=R.f32v(0.1), reduction="none") + c32 * torch.logsumexp(leaf, -1) ** 2
    (g2,) = torch.autograd.grad(ref.sum() * s32, leaf)
    ref = ref.detach()
    assert float((both["obj"][ok] - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    assert float((both["dlogits"][ok][:, :V] - g2).abs().max()) <= 1e-12


@pytest.mark.parametrize("model", [False, True])
@pytest.mark.parametrize("kind,bf16,rows", [("normal3", False, None), ("bf16x5", True, None), ("shift-3000", False, "rows")])
def test_options_off_is_rowwise_ref_exactly(model, kind, bf16, rows):
    rows = None if rows is None else [(7 * i + 3) % 50 for i in range(N)]
    z = R.ce_logits(N if rows is None else 50, V, LDL, kind, bf16)
    t = R.ce_targets(N, V, LDL)
    for ldd in (LDL, 1004, LDL + 8):
        a = LO.cross_entropy_opt(z, rows, t, V, SCALE, ldd, model=model)
        b = R.cross_entropy(z, rows, t, V, SCALE, ldd, model=model)
        for k in ("nll", "loss", "dlogits"):
            assert torch.equal(a[k], b[k]), (k, ldd)
        assert torch.equal(a["obj"], b["nll"])


def test_model_mean_survives_a_shift():
    """The f32 model's smoothing term on logits near -3000 is as accurate as on the same row near 0 (the shifted sum); a mean of the raw
    f32 logits would be off by the rounding of a sum of 1003 values of size 3000."""
    z, t = _case("shift-3000")
    e, m = LO.cross_entropy_opt(z, None, t, V, 1.0, LDL, eps=0.9), LO.cross_entropy_opt(z, None, t, V, 1.0, LDL, eps=0.9, model=True)
    err = float((m["obj"] - e["obj"]).abs().max())
    assert err <= 4 * 2.0 ** -24 * 3000.0, err                      # a few roundings of lse (|lse| ~ 3000), nothing that grows with V
    naive = float(np.abs(np.float32(z[:, :V].numpy().astype(np.float32).sum(-1, dtype=np.float32)) / np.float32(V)
                         - z[:, :V].double().mean(-1).numpy()).max())
    print(f"LOSSOPT model error {err:.3e}; a raw f32 mean alone would be off by up to {naive:.3e}")

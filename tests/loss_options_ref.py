"""CPU float64 reference of the LM loss options of csrc/loss.hip (include/ta355.h ``ta_ce_options``: label smoothing eps and z-loss
zc inside the cross-entropy launch) and its f32 model twin, in the style of ``rowwise_ref.cross_entropy``: ONE function evaluated in
the two arithmetics of tests/rowwise_ref.py (``model=False`` exact float64 from the bits the kernel gets, ``model=True`` every
elementwise operation rounded to f32 and every reduction accumulated left to right in f32).  The gates are rowwise_ref's, imported.

Per row r with a valid target t, over the V true columns (hyper-parameters: their f32 bits, as a C ``float`` argument carries them):
    lse  = m + log(sum_v exp(z_v - m)),  m = max_v z_v
    nll  = lse - z_t
    obj  = (1 - eps) nll + eps ((lse - c) - sum_v (z_v - c) / V) + zc lse lse,      c = z_0
    loss = sum_r obj_r * scale, rows in index order
    dlogits_v = p_v k1 - k2 - k3 [v == t],   p_v = exp(z_v - lse),  k1 = scale (1 + 2 zc lse),  k2 = scale eps / V,  k3 = scale (1 - eps)
which is   scale (p_v (1 + 2 zc lse) - (1 - eps) [v == t] - eps / V),   the gradient of scale * obj  (tests/test_loss_options_ref.py
ties it to float64 autograd of torch.nn.functional.cross_entropy(label_smoothing=eps) and of zc * logsumexp^2).  In exact arithmetic
c drops out: the smoothing term is lse - mean_v z_v whatever c is; in f32 the shifted sum keeps a row of logits near -3000 from
losing its mean to cancellation, so the model, too, is stated with it.  Rows of invalid targets: nll = obj = 0 and a zero dlogits row;
columns >= V: exact zeros.  eps = zc = 0 reproduces ``rowwise_ref.cross_entropy`` bit for bit in both arithmetics.
"""
import torch

from tests import rowwise_ref as R

OPTIONS = ((0.1, 0.0), (0.0, 1e-4), (0.1, 1e-4), (0.9, 1e-2))


def cross_entropy_opt(logits, rows, targets, V, scale, ldd, eps=0.0, zc=0.0, model=False):
    """ta_cross_entropy_opt.  Arguments as ``rowwise_ref.cross_entropy`` plus the two options.  -> nll [n] (plain, 0 on invalid rows),
    obj [n], loss = sum_i obj_i * scale in row order, dlogits [n, ldd] before the bf16 rounding, lse [n], valid [n]."""
    A = R._Arith(model)
    n = len(targets)
    idx = torch.arange(n) if rows is None else torch.tensor(rows, dtype=torch.long)
    z = A.t(logits)[idx][:, :V]
    t = torch.tensor(targets, dtype=torch.long)
    valid = (t >= 0) & (t < V)
    tc = torch.where(valid, t, torch.zeros_like(t))
    sc, e, c2 = A.t(scale), A.t(eps), A.t(zc)
    one, zero, Vf = A.c(1.0), torch.zeros((), dtype=A.dt), A.c(float(V))
    m = z.amax(-1)
    lse = m + A.log(A.sum(A.exp(z - m[:, None])))
    nll = torch.where(valid, lse - z.gather(1, tc[:, None])[:, 0], zero)
    c = z[:, 0]
    smooth = (lse - c) - A.sum(z - c[:, None]) / Vf
    obj = torch.where(valid, (one - e) * nll + e * smooth + c2 * lse * lse, zero)
    loss = A.sum(obj * sc, 0)
    k1, k2, k3 = sc * (one + A.c(2.0) * c2 * lse), sc * e / Vf, sc * (one - e)
    d = A.exp(z - lse[:, None]) * k1[:, None] - k2
    d[torch.arange(n), tc] -= k3
    d = d * valid[:, None].to(A.dt)
    dl = torch.zeros(n, ldd, dtype=A.dt)
    dl[:, :min(V, ldd)] = d[:, :min(V, ldd)]
    return R._out(nll=nll, obj=obj, loss=loss, dlogits=dl, lse=lse, valid=valid)


def objective(logits, labels, eps=0.0, zc=0.0, num_items=None):
    """The objective of a [B, L, V] logits tensor and [B, L] labels (shifted, ignore -100) in float64, differentiable:
    sum over the label tokens of (1 - eps) nll + eps (lse - mean_v z) + zc lse^2, divided by ``num_items`` (default: their number).
    What ASRModel.forward(labels=..., label_smoothing=eps, z_loss_coef=zc) returns as ``loss``."""
    z = logits[:, :-1].reshape(-1, logits.shape[-1]).to(torch.float64)
    t = labels[:, 1:].reshape(-1)
    keep = t != -100
    z, t = z[keep], t[keep]
    lse = torch.logsumexp(z, -1)
    nll = lse - z.gather(1, t[:, None])[:, 0]
    obj = (1.0 - eps) * nll + eps * (lse - z.mean(-1)) + zc * lse * lse
    return obj.sum() / float(num_items if num_items is not None else max(int(keep.sum()), 1))

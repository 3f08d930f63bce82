"""Host tests of tests/moe_ref.py (CPU, float64): the reference the GPU grid (tests/test_gpu_moe_grid.py) is measured against.

  * the exact form against the numpy oracle (oracle/projectors.py, fp32) and against the vectors the original implementation produced
    (tests/golden/projector_moe.npz): forward, aux, every gradient, within the oracle's fp32 noise;
  * the hand-written backward with rounding off equals float64 autograd;
  * every grid case meets its target slot counts and its routing-margin condition (and which cases needed more than one seed);
  * planted single-site errors each fail the gate on the outputs they touch, so the gate has power where the old cosine gates had none.
"""
import numpy as np
import pytest
import torch

from oracle import projectors as OP
from oracle import weights as OW
from tests import moe_ref as M
from tests.golden import recipe as R

F64 = torch.float64


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))


def small_setup():
    """The golden vectors' configuration (enc 256, k 4, hidden 128, llm 256, E 4); x through bf16, as the reference reads bf16 bits."""
    E, D, H = R.SMALL["enc"]["hidden"], R.SMALL["lm"]["hidden"], R.SMALL["proj_hidden"]
    w = OW.init_moe_projector(E, D, H)
    x, dy = R.proj_input()
    return w, {n: torch.from_numpy(v) for n, v in w.items()}, x, dy


# the oracle runs in fp32: products over In = 1024 terms, and gradients that sum 24 tokens of them; 1e-4 of the largest element is
# the bound tests/test_oracle_golden.py already holds the oracle itself to against the same vectors
ORACLE_TOL = 1e-4


@pytest.mark.parametrize("training,d_aux", [(False, 0.0), (True, 3.0)])
def test_exact_form_vs_oracle(training, d_aux):
    """Same bf16-representable input to both: the oracle in fp32, the reference in float64."""
    w, W, x, dy = small_setup()
    xb = torch.from_numpy(x).to(torch.bfloat16)
    rng = np.random.RandomState(4)
    noise = rng.uniform(0.99, 1.01, size=(24, 4)).astype(np.float32) if training else None
    y, aux, c = OP.moe_forward(xb.float().numpy(), w, training=training, jitter_noise=noise)
    go = OP.moe_backward(dy, w, c, d_aux=d_aux)
    f, g = M.backward_exact(xb, W, torch.from_numpy(dy), d_aux, 4, 4, training=training, noise=None if noise is None else torch.from_numpy(noise))
    assert np.array_equal(np.sort(c["order"], -1), f["topi"].sort(-1).values.numpy())
    assert relerr(f["y"].numpy().reshape(y.shape), y) < 1e-5
    assert abs(float(f["aux"]) - float(aux)) < 1e-6 * max(1.0, abs(float(aux)))
    for n in w:
        assert relerr(g[n].numpy(), go[n]) < ORACLE_TOL, n


def test_exact_form_vs_golden(golden):
    """The vectors of the original implementation were made from the f32 x (no bf16 rounding): the reference takes float input too."""
    gold = golden("projector_moe.npz")
    w, W, x, dy = small_setup()
    xt, dyt = torch.from_numpy(x).to(F64), torch.from_numpy(dy)
    f, g = M.backward_exact(xt, W, dyt, 0.0, 4, 4, training=False)
    assert relerr(f["y"].numpy().reshape(gold["y_eval"].shape), gold["y_eval"]) < 1e-5 and float(f["aux"]) == float(gold["aux_eval"]) == 0.0
    for n in [k[3:] for k in gold.files if k.startswith("ge.")]:
        assert relerr(g[n].numpy(), gold["ge." + n]) < ORACLE_TOL, n
    f, g = M.backward_exact(xt, W, dyt, 3.0, 4, 4, training=True)
    assert relerr(f["y"].numpy().reshape(gold["y_train"].shape), gold["y_train"]) < 1e-5
    assert abs(float(f["aux"]) - float(gold["aux_train"])) < 1e-6 * max(1.0, abs(float(gold["aux_train"])))
    for n in w:
        assert relerr(g[n].numpy(), gold["gt." + n]) < ORACLE_TOL, n


@pytest.mark.parametrize("cid", ["T5-E4-noise", "T65-E4-zeroframes", "T64-E8-train", "T63-E4-onepair-eval"])
def test_hand_backward_equals_autograd(cid):
    """Rounding off: the restated kernel formulas are the derivative (float64: 1e-10 of each tensor's largest element)."""
    r = M.ref(cid); c = r.c
    f, g = M.backward_model(r.I["x"], r.I["W"], r.I["dy"], c.d_aux, M.K, c.E, rounded=False, **r.kw)
    assert torch.equal(f["y"], r.fx["y"]) and float(f["aux"]) == float(r.fx["aux"])
    for n in r.gx:
        assert float((g[n] - r.gx[n]).abs().max()) <= 1e-10 * max(float(r.gx[n].abs().max()), 1e-30), n


@pytest.mark.parametrize("cid", M.ALL)
def test_grid_case_routing(cid):
    """Every case: the target counts, the margin of every non-zero token, the same routing in both forms; zero-frame tokens on (0, 1)."""
    r = M.ref(cid); c = r.c
    print(f"MOECASE {cid} seeds drawn={r.tries} {r.fig}")
    assert r.ok and r.fig["counts"] == list(c.counts) and r.fig["min_margin"] > 1.0 and r.fig["same"]
    assert int(r.I["zero"].sum()) == c.n_zero
    assert r.fx["y"].shape == (c.T, c.D) and r.I["x"].shape == (c.B, c.S, M.ENC)
    if c.extra:
        assert c.S % M.K != 0


# ----------------------------------------------------------------------------- planted errors
PLANT = "T65-E4-zeroframes"          # training, d_aux = 3, four experts all in use: every planted site exists


def _planted(inject, r):
    c = r.c
    f, g = M.backward_model(r.I["x"], r.I["W"], r.I["dy"], c.d_aux, M.K, c.E, rounded=False, inject=inject, **r.kw)
    return f, g


def _fails(r, name, bad):
    if name == "y":
        return not M.gate(bad, r.fx["y"], r.fm["y"], width=r.c.D)[0]
    return not M.gate(bad, r.gx[name], r.gm[name], width=M.width_of(name, r.gx[name]))[0]


def test_planted_third_expert():
    r = M.ref(PLANT)
    t = int((~r.I["zero"]).nonzero()[0])
    a, b = (int(i) for i in r.fx["topi"][t])
    third = int(torch.argsort(-r.fx["probs"][t], stable=True)[2])
    f, g = _planted({"third_expert": t}, r)
    assert _fails(r, "y", f["y"])
    for e in (b, third):
        for s in ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"):
            assert _fails(r, f"experts.{e}.{s}", g[f"experts.{e}.{s}"]), (e, s)
    assert _fails(r, "router.weight", g["router.weight"])


@pytest.mark.parametrize("cid,e", [(PLANT, 2), ("T512-E8-noise", 3), ("T1100-E8-skew-train", 5)])
def test_planted_last_slot_dropped(cid, e):
    """The last slot of one expert's segment (count 35, 64, 65) left out of that expert's four parameter gradients."""
    r = M.ref(cid)
    f, g = _planted({"drop_last_slot": e}, r)
    for s in ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"):
        assert _fails(r, f"experts.{e}.{s}", g[f"experts.{e}.{s}"]), s


def test_planted_no_renormalisation():
    r = M.ref(PLANT)
    t = int((~r.I["zero"]).nonzero()[1])
    f, g = _planted({"no_renorm": t}, r)
    assert _fails(r, "y", f["y"])


def test_planted_missing_aux_share():
    """One token's dlogits without the auxiliary share: shows in router.weight (and through dxn in norm.weight) when the loss is the
    auxiliary one -- the share ta_moe_router_aux_grads returns on its own."""
    r = M.ref(PLANT); c = r.c
    dy0 = torch.zeros_like(r.I["dy"])
    _, gx = M.backward_exact(r.I["x"], r.I["W"], dy0, c.d_aux, M.K, c.E, **r.kw)
    _, gm = M.backward_model(r.I["x"], r.I["W"], dy0, c.d_aux, M.K, c.E, rounded=True, **r.kw)
    t = int((~r.I["zero"]).nonzero()[2])
    _, gb = M.backward_model(r.I["x"], r.I["W"], dy0, c.d_aux, M.K, c.E, rounded=False, inject={"no_aux_token": t}, **r.kw)
    for n in ("router.weight", "norm.weight"):
        assert not M.gate(gb[n], gx[n], gm[n], width=M.width_of(n, gx[n]))[0], n


def test_planted_tail_rstd_from_neighbour():
    r = M.ref("T5-E4-noise")
    f, g = _planted({"rstd_from_neighbour": True}, r)
    assert _fails(r, "y", f["y"])
    ok, _, worst = M.gate(f["y"], r.fx["y"], r.fm["y"], width=r.c.D)
    assert worst == r.c.T - 1


def test_aux_gate():
    """The scalar gate passes the model itself and fails an aux whose balance term misses one token's probabilities."""
    r = M.ref(PLANT); c = r.c
    ex, mo = float(r.fx["aux"]), float(r.fm["aux"])
    f32 = M.aux_f32(r.fm, c.E, M.COEF, M.ZCOEF)
    assert M.gate_aux(mo, ex, mo, f32)[0] and M.gate_aux(f32, ex, mo, f32)[0]
    keep = torch.ones(c.T, dtype=torch.bool); keep[7] = False
    bad = float(M.aux_loss(r.fx["probs"][keep] * (c.T - 1) / c.T, r.fx["lse"], c.E, M.COEF, M.ZCOEF))
    assert not M.gate_aux(bad, ex, mo, f32)[0]
    assert M.gate_aux(0.0, 0.0, 0.0, 0.0)[0] and not M.gate_aux(1e-9, 0.0, 0.0, 0.0)[0]

"""Host tests of tests/attention_ref.py: the float64 reference of the LM attention block and the per-row gate
(max_r e_r <= 2 max_r m_r) that tests/test_gpu_attention_grid.py applies to every attention entry point.  No GPU.

  * the exact reference agrees with torch's scaled_dot_product_attention (float64) and with transformers' eager Qwen3 attention block;
  * its hand-written backward (the kernels' formulas) equals autograd when nothing is rounded;
  * the gate catches what it is for: three single-row errors injected into the REFERENCE fail it for O and every gradient.
"""
import functools

import pytest
import torch

from tests import attention_ref as R

B, HQ, HKV = 2, 4, 2


def test_exact_reference_matches_sdpa_float64():
    L = 70
    I = R.make_inputs(L, HQ, HKV, seed=1)
    km = torch.ones(B, L, dtype=torch.int32); km[1, L - 9:] = 0
    f = R.forward(I["qkv0"], B, L, HQ, HKV, kmask=km)                       # no norm, no RoPE: Q, K, V are the input's bits
    q, k, v = f["Q"], f["K"].repeat_interleave(2, 1), f["V"].repeat_interleave(2, 1)
    ref = torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=f["vis"][:, None])
    ref = ref.transpose(1, 2).reshape(B * L, HQ * R.HD)
    assert float((f["O"] - ref).abs().max()) < 1e-12
    s = (q @ k.transpose(-1, -2)) * R.HD ** -0.5
    lse = torch.logsumexp(s.masked_fill(~f["vis"][:, None], float("-inf")), -1)
    assert float((f["LSE"] - lse).abs().max()) < 1e-12


class _Float64Torch:
    """``torch`` as transformers' modeling file sees it, with float32 reading float64: Qwen3RMSNorm and eager_attention_forward upcast
    to ``torch.float32`` by name, which in a float64 run is a DOWNcast (4e-7 on O).  Everything else is torch itself."""
    float32 = torch.float64

    def __getattr__(self, name):
        return getattr(torch, name)


def test_exact_reference_matches_transformers_eager_qwen3_attention(monkeypatch):
    tf = pytest.importorskip("transformers")
    from transformers.models.qwen3 import modeling_qwen3
    from transformers.models.qwen3.modeling_qwen3 import Qwen3Attention
    monkeypatch.setattr(modeling_qwen3, "torch", _Float64Torch())
    L, hid = 40, (HQ + 2 * HKV) * R.HD
    I = R.make_inputs(L, HQ, HKV, seed=2)
    km = torch.ones(B, L, dtype=torch.int32); km[0, L - 7:] = 0
    pos = (torch.arange(L)[None] + torch.tensor([[100], [3]])).to(torch.int32)          # table rows that are not the row index
    f = R.forward(I["qkv0"], B, L, HQ, HKV, qn_w=I["qn_w"], kn_w=I["kn_w"], cos=I["cos"], sin=I["sin"], pos=pos, kmask=km)
    cfg = tf.Qwen3Config(hidden_size=hid, num_attention_heads=HQ, num_key_value_heads=HKV, head_dim=R.HD, rms_norm_eps=R.EPS,
                         attention_bias=False, attention_dropout=0.0, num_hidden_layers=1, vocab_size=8, intermediate_size=8)
    cfg._attn_implementation = "eager"
    att = Qwen3Attention(cfg, layer_idx=0).to(torch.float64).eval()
    eye = torch.eye(hid, dtype=torch.float64)
    with torch.no_grad():                                                    # the projections select the q | k | v columns of the input
        att.q_proj.weight.copy_(eye[:HQ * R.HD]); att.k_proj.weight.copy_(eye[HQ * R.HD:(HQ + HKV) * R.HD])
        att.v_proj.weight.copy_(eye[(HQ + HKV) * R.HD:]); att.o_proj.weight.copy_(eye[:, :HQ * R.HD])
        att.q_norm.weight.copy_(I["qn_w"].double()); att.k_norm.weight.copy_(I["kn_w"].double())
    c, s = I["cos"].double()[pos.long()], I["sin"].double()[pos.long()]
    emb = (torch.cat([c, c], -1), torch.cat([s, s], -1))
    add = torch.zeros(B, 1, L, L, dtype=torch.float64).masked_fill(~f["vis"][:, None], float("-inf"))
    with torch.no_grad():
        out = att(I["qkv0"].double().reshape(B, L, hid), position_embeddings=emb, attention_mask=add)[0]
    got = out.reshape(B * L, hid)[:, :HQ * R.HD]
    assert float((f["O"] - got).abs().max()) < 1e-10


# ----------------------------------------------------------------------------- the case [63, 2, 63, 64]
L192 = 192


@functools.lru_cache(maxsize=None)
def packed_case():
    I = R.make_inputs(L192, HQ, HKV, seed=0)
    sid = R.segment_ids_of([[63, 2, 63, 64], [40, 100]], L192)           # row 1 ends in 52 padding tokens
    km = (sid != 0).int()
    kw = dict(qn_w=I["qn_w"], kn_w=I["kn_w"], cos=I["cos"], sin=I["sin"], pos=R.segment_positions(sid), kmask=km, segment_ids=sid)
    dO = R.mask_dO(I["dO"], km, B, L192)
    fwd, dQ, dK, dV, dx = R.backward_exact(I["qkv0"], dO, B, L192, HQ, HKV, **kw)
    exact = dict(O=fwd["O"], Q=fwd["Q"], K=fwd["K"], dQ=dQ, dK=dK, dV=dV, dqkv=dx)
    m = R.backward_model(I["qkv0"], dO, B, L192, HQ, HKV, rounded=True, **kw)
    model = dict(O=m["fwd"]["O"], Q=m["fwd"]["Q"], K=m["fwd"]["K"], dQ=m["dQ"], dK=m["dK"], dV=m["dV"], dqkv=m["dqkv_fused"])
    return I, kw, dO, fwd, exact, model


def test_handwritten_backward_equals_autograd_when_nothing_is_rounded():
    I, kw, dO, fwd, exact, _ = packed_case()
    m = R.backward_model(I["qkv0"], dO, B, L192, HQ, HKV, rounded=False, **kw)
    for name, key in (("dQ", "dQ"), ("dK", "dK"), ("dV", "dV"), ("dqkv", "dqkv_fused"), ("dqkv", "dqkv_unfused")):
        assert float((m[key] - exact[name]).abs().max()) < 1e-12, key


def test_rounding_model_is_close_to_exact_and_padding_is_zero():
    """The two forms differ by bf16 roundings only (every row within a few 2^-8 of exact, save rows that are ~0 by cancellation), and
    rows with no visible key are exactly 0 in both."""
    I, kw, dO, fwd, exact, model = packed_case()
    for name in ("O", "Q", "K", "dK", "dV"):
        assert float(R.row_errors(model[name], exact[name]).max()) < 2e-2, name
    for name in ("dQ", "dqkv"):
        assert float(R.row_errors(model[name], exact[name]).median()) < 1e-2, name
    none = ~fwd["vis"].any(-1)                                              # [B, L]
    assert bool(none.any())
    for d in (exact, model):
        assert not d["O"].reshape(B, L192, -1)[none].any()
        assert not d["dqkv"].reshape(B, L192, -1)[none].any()
    assert torch.isinf(fwd["LSE"].transpose(1, 2)[none]).all()


def _perturbed(vis=None, pos_q=None):
    I, kw, dO, fwd, exact, _ = packed_case()
    m = R.backward_model(I["qkv0"], dO, B, L192, HQ, HKV, rounded=False, vis=vis, pos_q=pos_q, **kw)
    return dict(O=m["fwd"]["O"], Q=m["fwd"]["Q"], K=m["fwd"]["K"], dQ=m["dQ"], dK=m["dK"], dV=m["dV"], dqkv=m["dqkv_fused"])


def _assert_fails_gate(bad, names=("O", "dQ", "dK", "dV", "dqkv")):
    _, _, _, _, exact, model = packed_case()
    for name in names:
        ok, ratio, worst = R.gate(bad[name], exact[name], model[name])
        print(f"{name}: max e / max m = {ratio:.2f} (worst row {worst})")
        assert not ok, (name, ratio)
    for name in exact:                                                      # ... and the unperturbed model passes, with room
        ok, ratio, _ = R.gate(model[name], exact[name], model[name])
        assert ok and ratio == 1.0


def test_gate_catches_a_segment_start_that_sees_the_previous_token():
    """seg[q] one too small at one row: row 65 (first token of segment 3 of batch row 0) also sees key 64."""
    vis = packed_case()[3]["vis"].clone()
    assert not vis[0, 65, 64] and vis[0, 65].sum() == 1
    vis[0, 65, 64] = True
    _assert_fails_gate(_perturbed(vis=vis))


def test_gate_catches_one_dropped_diagonal():
    """One row loses its own key: row 105 of batch row 0, the 41st token of a 63-token segment (softmax weight ~ 1/41 on average:
    the least visible single-key error the layout offers short of the segment's last rows)."""
    vis = packed_case()[3]["vis"].clone()
    assert vis[0, 105, 105] and vis[0, 105].sum() == 41
    vis[0, 105, 105] = False
    _assert_fails_gate(_perturbed(vis=vis))


def test_gate_catches_rope_rows_taken_from_the_row_index():
    """The table row of the QUERY side comes from the row index where ``pos`` was meant (the fused forward loads the query-side and the
    key-side rows separately).  Taking the row index on BOTH sides shifts q and k of a segment by the same angle, which leaves q.k,
    hence O and d(qkv0), unchanged for every ``pos`` that is a per-segment shift of the row index (all the forms a batch passes): that
    error shows in Q, K, dQ and dK only, which the grid compares directly -- asserted second."""
    rowidx = torch.arange(L192, dtype=torch.int32)[None].expand(B, L192)
    _assert_fails_gate(_perturbed(pos_q=rowidx))
    I, kw, dO, _, exact, model = packed_case()
    kw2 = dict(kw, pos=rowidx)
    m = R.backward_model(I["qkv0"], dO, B, L192, HQ, HKV, rounded=False, **kw2)
    both = dict(Q=m["fwd"]["Q"], K=m["fwd"]["K"], dQ=m["dQ"], dK=m["dK"])
    for name in both:
        ok, ratio, _ = R.gate(both[name], exact[name], model[name])
        assert not ok, (name, ratio)
    # the invariance stated above, up to the f32 rounding of the table entries (rows p and p + c are not an exact rotation apart)
    assert float((m["fwd"]["O"] - exact["O"]).abs().max()) < 1e-5


# ----------------------------------------------------------------------------- the gate's power in every case of the GPU grid
from tests import test_gpu_attention_grid as G  # noqa: E402  (imports no GPU code without a GPU)


@pytest.mark.parametrize("cid", G.ALL)
def test_grid_case_inputs_give_the_gate_its_power(cid):
    """For the inputs each grid case runs with, one dropped diagonal in the longest row and one extra key at a single-key row -- injected
    into the reference -- read at least POWER x the rounding model's worst row for dQ and d(qkv0), and fail the gate for O, dK and dV.
    max_r m_r of dQ depends heavily on the draw (one short, peaked row whose exact dQ nearly cancels can put it at 0.7), so
    test_gpu_attention_grid.ref draws each case's inputs until this holds; here the choice is re-derived and checked on the host."""
    r = G.ref(cid)
    sens = G.sensitivity(r)
    print(f"{cid}: seed {r.seed}, dQ diag {sens[('diag', 'dQ')]:.1f} extra {sens[('extra', 'dQ')]:.0f}, "
          f"d(qkv0) diag {sens[('diag', 'dqkv')]:.1f} extra {sens[('extra', 'dqkv')]:.0f}")
    assert G.powerful(sens), sens
    assert min(sens[(p, t)] for p in ("diag", "extra") for t in ("dQ", "dqkv")) >= G.POWER > 2.0

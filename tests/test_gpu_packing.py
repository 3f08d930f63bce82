"""Sequence packing on the device: several clips per LM row, block-diagonal causal attention (``segment_ids``), against the same
clips run ONE PER ROW on the CPU.  Truth: ``oracle.qwen3.lm_forward`` per segment for every token's logits and nll; transformers'
``Qwen3ForCausalLM`` / ``SmolLM3ForCausalLM`` in fp32, one clip per row, under ``functional_call`` + autograd for every gradient (adapter
gradients through W + s B A).  The library's own unpacked path is never the truth.

Gates are the ones the existing tests apply to the same quantities on the small configuration -- no new number:
  loss        |d| < 5e-3 * ref                         tests/test_gpu_round5.py:207 (position_ids), tests/test_gpu_parity.py:281
  logits      max|d| / max|ref| < 2e-2                 tests/test_gpu_round5.py:209-210 (position_ids / left padding)
  nll         |d| < 2 * (2e-2 * max|ref logits|)       nll = logsumexp(z) - z[t]: both terms move by at most the logits bound above
  d(audio)    cosine > 0.999                           tests/test_gpu_round5.py:249, tests/test_gpu_parity.py:288
  LoRA grads  cosine > 0.998 and relmax < 6e-2         tests/test_gpu_parity.py:355-356
  full FT     cosine > 0.995 and relmax < 6e-2         tests/test_gpu_parity.py:920
"""
import numpy as np
import pytest
import torch

from oracle import qwen3 as OQ
from oracle import weights as OW
from tests.golden import recipe as R

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tiny_audio_amd import ops
    from tiny_audio_amd.asr_config import ASRConfig, LMConfig
    from tiny_audio_amd.asr_modeling import ASRModel
    from tiny_audio_amd.asr_processing import LogMelFeatureExtractor
    from tiny_audio_amd.collator import DataCollator
    from tiny_audio_amd.language_model import Qwen3MI355X

DEV = "cuda"
# Lp = 192, KV tile 64: a boundary mid-tile (70) and one on a tile edge (128), the last segment wholly inside the third tile; a row that
# ends in 52 padding tokens; one segment that fills the row
ROWS_192 = [[70, 58, 64], [40, 100], [192]]
ROWS_320 = [[130, 190]]                      # beyond the fused forward's envelope (L <= 192): the tiled pair


def npy(t):
    return t.detach().float().cpu().numpy()


def cosine(a, b):
    a = np.asarray(a, np.float64).ravel(); b = np.asarray(b, np.float64).ravel()
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-30))


def relmax(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / (np.abs(b).max() + 1e-30))


# ----------------------------------------------------------------------------- batches and the CPU truth
def packed_batch(rows, D, vocab, seed=7):
    """-> x [R, Lp, D] inputs_embeds (zeros on padding), sid [R, Lp], lab [R, Lp] (the last third of every clip labelled; never the clip's
    first token), and the clips in packed order as (row, start, length)."""
    rng = np.random.RandomState(seed)
    Lp = max(sum(r) for r in rows)
    x = np.zeros((len(rows), Lp, D), np.float32)
    sid = np.zeros((len(rows), Lp), np.int32)
    lab = np.full((len(rows), Lp), -100, np.int64)
    clips = []
    for r, lens in enumerate(rows):
        at = 0
        for s, n in enumerate(lens):
            x[r, at:at + n] = rng.standard_normal((n, D)) / np.sqrt(D)
            sid[r, at:at + n] = s + 1
            lab[r, at + 2 * n // 3:at + n] = rng.randint(0, vocab - 1, n - 2 * n // 3)
            clips.append((r, at, n))
            at += n
    return x, sid, lab, clips


def hf_model(kind, cfg, w):
    import transformers
    geom = dict(vocab_size=cfg["vocab"], hidden_size=cfg["hidden"], intermediate_size=cfg["ffn"], num_hidden_layers=cfg["layers"],
                num_attention_heads=cfg["heads"], num_key_value_heads=cfg["kv_heads"], head_dim=cfg["head_dim"], max_position_embeddings=512,
                rms_norm_eps=cfg["rms_eps"], tie_word_embeddings=True, rope_parameters=dict(rope_type="default", rope_theta=cfg["rope_theta"]),
                pad_token_id=None, bos_token_id=1, eos_token_id=2)
    if kind == "qwen3":
        model = transformers.Qwen3ForCausalLM(transformers.Qwen3Config(**geom, attention_bias=False))
    else:
        geom.pop("head_dim")
        model = transformers.SmolLM3ForCausalLM(transformers.SmolLM3Config(**geom, no_rope_layers=[1] * (cfg["layers"] - 1) + [0]))
    res = model.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=False)
    assert not res.unexpected_keys and set(res.missing_keys) <= {"lm_head.weight"}, res
    model.tie_weights()
    model = model.float().eval()
    model.config._attn_implementation = "eager"
    return model


def truth(model, w, cfg, x, lab, clips, lora=None, lora_scale=0.0, oracle=True):
    """One clip per row on the CPU.  -> dict(logits [R, Lp, V] (oracle per segment), nll (packed label order), loss, dx [R, Lp, D],
    grads {parameter name: d(loss)} of the transformers model -- with ``lora``: of the adapter matrices)."""
    from torch.func import functional_call
    params = {k: v.detach().clone().requires_grad_(lora is None) for k, v in model.named_parameters()}
    lo = {k: torch.from_numpy(v).clone().requires_grad_(True) for k, v in (lora or {}).items()}
    def effective():                                  # W + s B A of every adapted linear: a fresh graph per clip
        eff = dict(params)
        for k in lo:
            if k.endswith("lora_A"):
                base = k[:-len(".lora_A")] + ".weight"
                eff[base] = params[base] + lora_scale * lo[k[:-1] + "B"] @ lo[k]
        return eff
    n_tot = int((lab != -100).sum())
    V = cfg["vocab"]
    out = dict(logits=np.zeros(x.shape[:2] + (V,), np.float32), dx=np.zeros_like(x), nll=[])
    total = 0.0
    for (r, at, n) in clips:
        xe = torch.from_numpy(x[r:r + 1, at:at + n]).requires_grad_(True)
        lg = functional_call(model, effective(), args=(), kwargs=dict(inputs_embeds=xe, use_cache=False)).logits[0].float()
        tl = torch.from_numpy(lab[r, at + 1:at + n])
        nll = torch.nn.functional.cross_entropy(lg[:-1], tl, ignore_index=-100, reduction="none")
        s = nll.sum() / n_tot
        g = torch.autograd.grad(s, [xe] + [p for p in list(params.values()) + list(lo.values()) if p.requires_grad], allow_unused=True)
        out["dx"][r, at:at + n] = g[0][0].numpy()
        names = [k for k, p in list(params.items()) + list(lo.items()) if p.requires_grad]
        for k, gg in zip(names, g[1:]):
            if gg is not None:
                out.setdefault("grads", {})
                out["grads"][k] = out["grads"].get(k, 0) + gg.numpy()
        out["nll"].append(nll[tl != -100].detach().numpy())
        total += float(s.detach())
        if oracle:          # the per-token truth of the issue: the unchanged oracle on the segment as its own row
            ol, _ = OQ.lm_forward(x[r:r + 1, at:at + n], np.ones((1, n), np.int64), w, cfg, keep_cache=False, lora=lora, lora_scale=lora_scale)
            out["logits"][r, at:at + n] = ol[0]
            on = torch.nn.functional.cross_entropy(torch.from_numpy(np.asarray(ol[0], np.float32))[:-1], tl, ignore_index=-100, reduction="none")
            out["nll"][-1] = on[tl != -100].numpy()
        else:
            out["logits"][r, at:at + n] = lg.detach().numpy()
    out["nll"], out["loss"] = np.concatenate(out["nll"]), total
    return out


def hip_packed(lm, x, sid, lab, with_seg=True):
    """The packed rows through ta_lm_forward_loss_seg / ta_lm_backward_seg, the inputs_embeds fed as <audio> rows."""
    Rr, Lp, Dm = x.shape
    ids = torch.full((Rr, Lp), lm.config.vocab_size - 1, dtype=torch.int64, device=DEV)
    src = torch.arange(Rr * Lp, dtype=torch.int32, device=DEV)
    s = torch.from_numpy(sid).to(DEV)
    seg, pos = ops.segment_table(s)
    rows, tg, n = ops.label_rows(torch.from_numpy(lab).to(DEV))
    n = int(n.item())
    loss, nll, logits, ctx = lm.forward_loss(ids, src, torch.from_numpy(x.reshape(Rr * Lp, Dm)).to(DEV), (s != 0).int().contiguous(), rows, tg, n,
                                             1.0 / n, want_logits=True, pos=pos, seg=seg if with_seg else None)
    d_audio, _, lg = lm.backward_from_ctx(ctx, Rr * Lp)
    torch.cuda.synchronize()
    return dict(loss=float(loss), nll=npy(nll)[:n], logits=npy(logits).reshape(Rr, Lp, -1)[:, :, :lm.config.vocab_size],
                dx=npy(d_audio).reshape(Rr, Lp, Dm), grads=lg, n=n)


def check(got, ref, sid, tag):
    real = sid != 0
    lmax = float(np.abs(ref["logits"][real]).max())
    dl = float(np.abs(got["logits"][real] - ref["logits"][real]).max()) / lmax
    dn = float(np.abs(got["nll"] - ref["nll"]).max())
    cs = cosine(got["dx"][real], ref["dx"][real])
    print(f"[packing] {tag}: loss {got['loss']:.5f} vs {ref['loss']:.5f}, logits relmax {dl:.4f}, nll max|d| {dn:.4f} (bound {2 * 2e-2 * lmax:.3f}), "
          f"d(audio) cosine {cs:.6f}")
    assert got["n"] == ref["nll"].size
    assert abs(got["loss"] - ref["loss"]) < 5e-3 * ref["loss"], tag
    assert dl < 2e-2, tag
    assert dn < 2 * 2e-2 * lmax, tag
    assert cs > 0.999, tag
    assert np.isfinite(got["logits"]).all() and np.isfinite(got["dx"]).all(), tag
    assert not got["dx"][~real].any(), tag              # padding rows receive no gradient at all


_CACHE = {}


def small(kind, heads, kv):
    """(config, weights, transformers model) of the SMALL configuration with the given GQA shape; SmolLM3: no q/k-norm, layer 1 NoPE."""
    key = (kind, heads, kv)
    if key not in _CACHE:
        cfg = dict(R.SMALL["lm"], heads=heads, kv_heads=kv)
        w = OW.init_lm(cfg, 1)
        if kind == "smollm3":
            cfg = dict(cfg, hidden=heads * 128)          # SmolLM3Config has no head_dim: hidden / heads
            w = {k: v for k, v in OW.init_lm(cfg, 1).items() if "q_norm" not in k and "k_norm" not in k}
        _CACHE[key] = (cfg, w, hf_model(kind, cfg, w))
    return _CACHE[key]


def truth_of(kind, heads, kv, rows):
    key = ("truth", kind, heads, kv, str(rows))
    if key not in _CACHE:
        cfg, w, model = small(kind, heads, kv)
        x, sid, lab, clips = packed_batch(rows, cfg["hidden"], cfg["vocab"])
        _CACHE[key] = (x, sid, lab, clips, truth(model, w, cfg, x, lab, clips, oracle=kind == "qwen3"))
    return _CACHE[key]


def hip_lm(kind, heads, kv, res_f32=False):
    cfg, w, model = small(kind, heads, kv)
    src = dict(model.config.to_dict())
    lm = Qwen3MI355X(LMConfig(src if kind == "smollm3" else cfg), DEV)
    lm.res_f32 = res_f32
    return lm.load_state_dict_hf(w)


# ============================================================================ 1. frozen LM: both forward paths, both groups, both stream modes
@pytest.mark.parametrize("res_f32", [False, True], ids=["bf16stream", "f32stream"])
@pytest.mark.parametrize("kind,heads,kv,rows", [("qwen3", 4, 2, ROWS_192), ("qwen3", 4, 1, ROWS_192), ("qwen3", 4, 2, ROWS_320),
                                                ("smollm3", 4, 1, ROWS_192), ("smollm3", 4, 1, [[40, 56], [96]])],
                         ids=["group2-fused", "group4-pair", "group2-L320-pair", "smollm3-group4-pair", "smollm3-group4-fused"])
def test_packed_rows_match_one_clip_per_row(kind, heads, kv, rows, res_f32):
    """Group 2 at Lp = 192 lies inside the fused forward's envelope (2 * ceil(192 / 32) = 12), group 4 outside it (24 > 12: q|k|v post
    kernel + tiled attention), Lp = 320 outside for every group; group 4 at Lp = 96 (4 * 3 = 12) is the fused kernel without PAIR."""
    x, sid, lab, clips, ref = truth_of(kind, heads, kv, rows)
    lm = hip_lm(kind, heads, kv, res_f32)
    if kind == "smollm3":
        assert lm._w.nope_layers != 0 and lm._layers_arr[0].qn_w is None
    got = hip_packed(lm, x, sid, lab)
    check(got, ref, sid, f"{kind} {heads}/{kv} {rows} res_f32={res_f32}")


def test_single_segment_row_matches_the_unpacked_call():
    """The 192-token row alone: packed (one segment) and through the plain entry points -- both within the gates of the same truth."""
    x, sid, lab, clips, ref = truth_of("qwen3", 4, 2, ROWS_192)
    one = dict(ref, logits=ref["logits"][2:], dx=ref["dx"][2:] * 1.0)
    n_tot, n_one = int((lab != -100).sum()), int((lab[2:] != -100).sum())
    one["nll"] = ref["nll"][-n_one:]
    one["loss"] = float(one["nll"].sum()) / n_one
    one["dx"] = one["dx"] * (n_tot / n_one)
    lm = hip_lm("qwen3", 4, 2)
    for with_seg in (True, False):
        check(hip_packed(lm, x[2:], sid[2:], lab[2:], with_seg=with_seg), one, sid[2:], f"single segment, seg={with_seg}")


def test_segment_ids_change_the_answer():
    """Without the table the second and third clips of a row attend to the clips before them: their logits must MISS the gate."""
    x, sid, lab, clips, ref = truth_of("qwen3", 4, 2, ROWS_192)
    got = hip_packed(hip_lm("qwen3", 4, 2), x, sid, lab, with_seg=False)
    later = sid > 1
    d = float(np.abs(got["logits"][later] - ref["logits"][later]).max()) / float(np.abs(ref["logits"][later]).max())
    print(f"[packing] no table: logits relmax on later segments {d:.4f}")
    assert d > 2e-2


# ============================================================================ 2. trainable LM
def test_packed_lora_gradients():
    """Rank 8 on all seven linears, lora_dropout 0: adapter gradients and d(audio) of the packed batch against one clip per row."""
    cfg, w, model = small("qwen3", 4, 2)
    x, sid, lab, clips = packed_batch(ROWS_192, cfg["hidden"], cfg["vocab"])
    lo = OW.init_lora(cfg, rank=8)
    ref = truth(model, w, cfg, x, lab, clips, lora=lo, lora_scale=4.0)
    lm = Qwen3MI355X(LMConfig(cfg), DEV).load_state_dict_hf(w)
    lm.enable_lora(rank=8, alpha=32).load_lora_state_dict(lo)
    got = hip_packed(lm, x, sid, lab)
    check(got, ref, sid, "lora r8")
    for p_, g_ in zip(lm.lora_parameters(), got["grads"]):
        p_.data.copy_(g_)
    mine = lm.export_lora_state_dict(prefix="model.", suffix="")
    assert set(mine) == set(ref["grads"])
    worst = min(cosine(npy(mine[k]), ref["grads"][k]) for k in mine)
    print(f"[packing] lora: worst adapter-gradient cosine {worst:.5f}")
    for k in mine:
        assert cosine(npy(mine[k]), ref["grads"][k]) > 0.998, k
        assert relmax(npy(mine[k]), ref["grads"][k]) < 6e-2, k


def test_packed_full_finetune_gradients():
    """Every LM weight trains (the trainable q_norm / k_norm take the un-fused attention backward): weight gradients and d(audio)."""
    cfg, w, model = small("qwen3", 4, 2)
    x, sid, lab, clips = packed_batch(ROWS_192, cfg["hidden"], cfg["vocab"])
    ref = truth(model, w, cfg, x, lab, clips)
    lm = Qwen3MI355X(LMConfig(cfg), DEV).load_state_dict_hf(w)
    lm.enable_full_finetune()
    got = hip_packed(lm, x, sid, lab)
    check(got, ref, sid, "full fine-tune")
    g = ref["grads"]
    L = cfg["layers"]
    lay = lambda i, n: g[f"model.layers.{i}.{n}.weight"]
    want = [np.stack([np.concatenate([lay(i, "self_attn.q_proj"), lay(i, "self_attn.k_proj"), lay(i, "self_attn.v_proj")]) for i in range(L)]),
            np.stack([lay(i, "self_attn.o_proj") for i in range(L)]),
            np.stack([np.concatenate([lay(i, "mlp.gate_proj"), lay(i, "mlp.up_proj")]) for i in range(L)]),
            np.stack([lay(i, "mlp.down_proj") for i in range(L)]),
            np.stack([lay(i, "input_layernorm") for i in range(L)]), np.stack([lay(i, "post_attention_layernorm") for i in range(L)]),
            np.stack([lay(i, "self_attn.q_norm") for i in range(L)]), np.stack([lay(i, "self_attn.k_norm") for i in range(L)]),
            g["model.norm.weight"], g["model.embed_tokens.weight"]]
    names = [k for k, _ in lm.FT_KINDS] + ["norm", "embed"]
    for name, mine, ref_g in zip(names, got["grads"], want):
        c, rm = cosine(npy(mine), ref_g), relmax(npy(mine), ref_g)
        print(f"[packing] full FT {name}: cosine {c:.5f} relmax {rm:.4f}")
        assert c > 0.995 and rm < 6e-2, (name, c, rm)


# ============================================================================ 3. the bookkeeping kernels, exact
def test_audio_index_seg_against_a_loop():
    AID, N = 99, 6
    sid = np.array([[1, 1, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 0, 0], [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2]], np.int32)
    ids = np.array([[5, AID, AID, AID, 7, 8, AID, AID, AID, AID, AID, 9, AID, AID], [AID] * 8 + [3, 4, AID, 5, AID, 6]], np.int64)
    counts = np.array([3, 5, 8, 1], np.int64)             # clip 2 asks for more than N rows; clip 3 has a surplus placeholder
    want = np.full(ids.shape, -1, np.int32)
    c0 = 0
    for r in range(2):
        for s in range(1, sid[r].max() + 1):
            j = 0
            for l in np.nonzero(sid[r] == s)[0]:
                if ids[r, l] == AID:
                    want[r, l] = (c0 + s - 1) * N + j if (j < N and j < counts[c0 + s - 1]) else -2
                    j += 1
        c0 += sid[r].max()
    T = lambda a: torch.from_numpy(a).to(DEV)
    got = npy(ops.audio_index_seg(T(ids), T(sid), T(counts), N, AID)).astype(np.int32).reshape(ids.shape)
    assert (got == want).all(), (got, want)
    assert (got[0, 12:] == -1).all() and got[1, 7] == -2 and got[1, 12] == -2


def test_segment_table_against_a_loop():
    sid = np.zeros((3, 200), np.int32)
    for r, lens in enumerate([[70, 58, 64], [40, 100], [200]]):
        at = 0
        for s, n in enumerate(lens):
            sid[r, at:at + n] = s + 1; at += n
    seg, pos = ops.segment_table(torch.from_numpy(sid).to(DEV))
    seg, pos = npy(seg).astype(np.int64).reshape(2, 3, 200), npy(pos).astype(np.int64).reshape(3, 200)
    for r in range(3):
        for l in range(200):
            same = np.nonzero(sid[r] == sid[r, l])[0]
            a, e, p = (same[0], same[-1] + 1, l - same[0]) if sid[r, l] else (l + 1, l, 0)
            assert (seg[0, r, l], seg[1, r, l], pos[r, l]) == (a, e, p), (r, l)


# ============================================================================ 4. padded query rows
def test_padding_rows_are_finite_and_take_no_gradient():
    """Attention backward alone on the row that ends in padding: dK / dV of padding keys exactly zero, outputs finite."""
    B, Hq, Hkv, L, hd = 1, 4, 2, 192, 128
    g = torch.Generator(device=DEV); g.manual_seed(3)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g).to(torch.bfloat16)
    Q, K, V, dO = rn(B, Hq, L, hd), rn(B, Hkv, L, hd), rn(B, Hkv, L, hd), rn(B * L, Hq * hd)
    sid = torch.zeros((1, L), dtype=torch.int32, device=DEV); sid[0, :40] = 1; sid[0, 40:140] = 2
    seg, _ = ops.segment_table(sid)
    km = (sid != 0).int().contiguous()
    VT = V.transpose(2, 3).contiguous()
    sc = hd ** -0.5
    O = torch.full((B * L, Hq * hd), 7.0, device=DEV, dtype=torch.bfloat16)        # pre-filled: a row nobody writes keeps its 7s
    O, lse = ops.attention_fwd_seg(Q, K, VT, L, sc, kmask=km, seg=seg, out=O)
    delta = (O.float() * dO.float()).reshape(L, Hq, hd).sum(-1).t().contiguous().reshape(B, Hq, L)
    dQ, dK, dV = torch.full_like(Q, 7), torch.full_like(K, 7), torch.full_like(V, 7)
    ops.attention_bwd_seg(Q, K, V, dO, lse, delta, L, sc, kmask=km, seg=seg, out=(dQ, dK, dV))
    torch.cuda.synchronize()
    assert torch.isfinite(O.float()).all() and torch.isfinite(dQ.float()).all()
    assert not O[140:].float().any() and not dQ[:, :, 140:].float().any()
    assert not dK[:, :, 140:].float().any() and not dV[:, :, 140:].float().any()
    assert dK[:, :, :140].float().abs().sum() > 0 and (dK.float() != 7).all()
    # the same forward against plain softmax attention inside each segment
    qf, kf, vf = Q.float(), K.float().repeat_interleave(2, 1), V.float().repeat_interleave(2, 1)
    s = (qf @ kf.transpose(2, 3)) * sc
    idx = torch.arange(L, device=DEV)
    ok = (sid[0][:, None] == sid[0][None, :]) & (sid[0][:, None] != 0) & (idx[None, :] <= idx[:, None])
    ref = torch.softmax(s.masked_fill(~ok, float("-inf")), -1).nan_to_num(0.0) @ vf
    got = O.float().reshape(L, Hq, hd).permute(1, 0, 2)[None]
    assert relmax(npy(got), npy(ref)) < 2e-2


# ============================================================================ 5. whole model
def test_whole_model_packed_batch_from_the_collator():
    """Five synthetic clips of unequal length through DataCollator(pack_to=192) and ASRModel.forward: loss and per-token nll against the
    oracle's one-clip-per-row values; the same batch WITHOUT ``segment_ids`` must move the nll of every non-first segment (on the parent
    commit the key is ignored, so this is the test that fails there)."""
    from oracle import model as OM
    from tests.test_packing_host import ToyTokenizer
    S = R.SMALL
    enc, lmc = OW.enc_config(256, 512, 1, 4), S["lm"]
    AID, PAD = S["audio_token_id"], S["pad_id"]
    wE, wL, wP = OW.init_encoder(enc, 0), OW.init_lm(lmc, 1), OW.init_mlp_projector(256, 256, 128)
    cfg = ASRConfig(audio_config=enc, text_config=lmc, projector_hidden_dim=128, audio_token_id=AID, pad_token_id=PAD, eos_token_id=S["eos_id"])
    m = ASRModel(cfg, device=DEV, init="none")
    m.audio_tower.load_state_dict_hf(wE); m.language_model.load_state_dict_hf(wL)
    m.load_state_dict({"projector." + k: torch.from_numpy(v) for k, v in wP.items()})
    fe = LogMelFeatureExtractor(128, DEV)
    tok = ToyTokenizer(AID, PAD)
    texts = ["a b c d e f", "g h i", "j k l m n o p q", "r s", "t u v w x"]
    feats = [dict(audio=dict(array=OW.synthetic_wave(i, n)), text=t) for i, (n, t) in enumerate(zip((16000, 9000, 21000, 6000, 12000), texts))]
    col = DataCollator(tok, lambda a, **kw: fe(a, sampling_rate=16000), 16000, projector=m.projector, pack_to=192)
    batch = col(feats)
    sid = batch["segment_ids"].numpy()
    assert sid.shape[1] <= 192 and sid.max() >= 2 and batch["input_features"].shape[0] == 5
    m.eval()
    with torch.no_grad():
        out = m(**batch, return_logits=False)
        out_wrong = m(**{k: v for k, v in batch.items() if k not in ("segment_ids", "position_ids")}, return_logits=False)
    # the oracle, one clip per row
    W = dict(encoder=wE, lm=wL, projector=wP)
    ocfg = dict(enc=enc, lm=lmc, projector_type="mlp", k=4, audio_token_id=AID)
    ids, lab = batch["input_ids"].numpy(), batch["labels"].numpy()
    ref_nll, later, c = [], [], 0
    for r in range(sid.shape[0]):
        for s in range(1, sid[r].max() + 1):
            cols = np.nonzero(sid[r] == s)[0]
            one = dict(input_ids=ids[r:r + 1, cols], attention_mask=np.ones((1, cols.size), np.int64), labels=lab[r:r + 1, cols],
                       input_features=npy(batch["input_features"][c:c + 1]), audio_token_counts=npy(batch["audio_token_counts"][c:c + 1]).astype(np.int64))
            ref = OM.asr_forward(one, W, ocfg, training=False)
            lg = torch.from_numpy(np.asarray(ref["logits"][0], np.float32))
            tl = torch.from_numpy(lab[r, cols][1:])
            nll = torch.nn.functional.cross_entropy(lg[:-1], tl, ignore_index=-100, reduction="none")[tl != -100].numpy()
            ref_nll.append(nll); later.append(np.full(nll.size, s > 1)); c += 1
    ref_nll, later = np.concatenate(ref_nll), np.concatenate(later)
    got, wrong = npy(out.nll), npy(out_wrong.nll)
    lmax = max(float(np.abs(np.asarray(OM.asr_forward(one, W, ocfg, training=False)["logits"])).max()), 1.0)
    print(f"[packing] whole model: loss {float(out.loss):.5f} vs {ref_nll.mean():.5f}, nll max|d| {np.abs(got - ref_nll).max():.4f}; "
          f"without segment_ids max|d| on later segments {np.abs(wrong - ref_nll)[later].max():.4f}")
    assert got.size == ref_nll.size and later.any()
    assert abs(float(out.loss) - ref_nll.mean()) < 5e-3 * ref_nll.mean()
    assert np.abs(got - ref_nll).max() < 2 * 2e-2 * lmax
    assert (np.abs(wrong - got)[later] > 0).all()

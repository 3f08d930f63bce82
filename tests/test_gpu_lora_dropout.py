"""LoRA dropout (peft ``lora_dropout`` p > 0) on the device: the mask definition, the masked kernels against torch fp32 with the
masks materialised, the reference fixture tests/golden/lora_dropout_small.npz, reproducibility and stage-2 training."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import weights as OW
from tests.golden import recipe as R
from tiny_audio_amd import lora_dropout as LD

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tiny_audio_amd import _lib, ops
    from tiny_audio_amd.asr_config import LMConfig
    from tiny_audio_amd.language_model import FrozenLMLoss, Qwen3MI355X
    from tiny_audio_amd.ops import ptr, stream

DEV = "cuda"


def cosine(a, b):
    a = np.asarray(a, np.float64).ravel(); b = np.asarray(b, np.float64).ravel()
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-30))


def npy(t):
    return t.detach().float().cpu().numpy()


def device_keep(p, seed, offset, layer, linear, M, n):
    out = torch.empty((M, n), dtype=torch.uint8, device=DEV)
    d = _lib.LoraDropout(p=p, seed=seed, offset=offset)
    _lib.check(_lib.lib().ta_lora_dropout_keep(C.byref(d), layer, linear, M, n, ptr(out), stream()), "ta_lora_dropout_keep")
    return out.cpu().numpy().astype(bool)


@pytest.mark.parametrize("p,seed,offset,layer,linear,M,n", [(0.1, 1234, 5, 0, 0, 96, 256), (0.3, 2 ** 62 + 7, (3 << 32) + 2, 27, 6, 77, 203),
                                                            (0.05, 1, 0, 5, 4, 6144, 40), (0.5, 99, 11, 1, 2, 33, 3072)])
def test_keep_mask_matches_numpy_twin(p, seed, offset, layer, linear, M, n):
    got = device_keep(p, seed, offset, layer, linear, M, n)
    np.testing.assert_array_equal(got, LD.keep_mask(p, seed, offset, layer, linear, M, n))
    assert device_keep(0.0, seed, offset, layer, linear, 5, n).all()


# ---------------------------------------------------------------------------- helpers: one LM with adapters, inputs_embeds as "audio"
def _lm(cfg, rank, alpha, targets, p, lo, wL):
    lm = Qwen3MI355X(LMConfig(cfg), DEV).load_state_dict_hf(wL)
    lm.enable_lora(rank=rank, alpha=alpha, dropout=p, target_modules=None if targets is None else list(targets)).load_lora_state_dict(lo)
    return lm


def _run(lm, x, att, lab, drop):
    B, L, D = x.shape
    ids = torch.full((B, L), lm.config.vocab_size - 1, dtype=torch.int64, device=DEV)
    src = torch.arange(B * L, dtype=torch.int32, device=DEV)
    rows, tg, n = ops.label_rows(torch.from_numpy(lab).to(DEV))
    n = int(n.item())
    audio = torch.from_numpy(x.reshape(B * L, D)).to(DEV)
    loss, _, _, ctx = lm.forward_loss(ids, src, audio, torch.from_numpy(att).to(DEV).int(), rows, tg, n, 1.0 / n, lora_dropout=drop)
    d_audio, _, lg = lm.backward_from_ctx(ctx, B * L)
    return float(loss), d_audio, lg


def _adapters(cfg, rank, targets):
    """the fixture's adapters (tests/golden/make_lora_dropout_fixture.py): oracle init_lora's A, a deterministic NON-zero B"""
    lo = OW.init_lora(cfg, rank=rank, seed=4, targets=targets)
    for i, k in enumerate(sorted(lo)):
        if k.endswith(".lora_B"):
            lo[k] = (np.random.RandomState(100 + i).standard_normal(lo[k].shape) * 0.05).astype(np.float32)
    return lo


def _grads_by_name(lm, lg):
    for p_, g_ in zip(lm.lora_parameters(), lg):
        p_.data.copy_(g_)
    return {k: npy(v) for k, v in lm.export_lora_state_dict(prefix="model.", suffix="").items()}


@pytest.mark.parametrize("pre,targets", [("c0", None), ("c1", ("q_proj", "v_proj"))])
def test_lora_dropout_vs_golden(golden, pre, targets):
    """The reference's Qwen3 with per-linear masked adapters (numpy-twin masks): r = 8 on all 7 linears at p = 0.1, and r = 4 on q, v at
    p = 0.3 with an offset above 2^32; gates of test_lora_vs_golden_config."""
    g = golden("lora_dropout_small.npz")
    cfg = R.SMALL["lm"]
    rank, alpha, p = int(g[pre + ".rank"]), int(g[pre + ".alpha"]), float(g[pre + ".p"])
    seed, offset = int(g[pre + ".seed"]), int(g[pre + ".offset"])
    lm = _lm(cfg, rank, alpha, targets, p, _adapters(cfg, rank, targets), OW.init_lm(cfg, seed=1))
    x, att, lab = R.lm_input()
    loss, d_audio, lg = _run(lm, x, att, lab, (p, seed, offset))
    assert abs(loss - float(g[pre + ".loss"])) < 5e-3 * float(g[pre + ".loss"])
    valid = att.astype(bool)
    assert cosine(npy(d_audio).reshape(x.shape)[valid], g[pre + ".dx"][valid]) > 0.999
    got = _grads_by_name(lm, lg)
    keys = [k[len(pre) + 3:] for k in g.files if k.startswith(pre + ".g.")]
    assert keys
    for k in keys:
        assert cosine(got[k], g[f"{pre}.g.{k}"]) > 0.998, k
    # the same model without dropout is measurably different: the masks are really applied
    loss0, d0, _ = _run(lm, x, att, lab, None)
    assert abs(loss0 - loss) > 1e-4 * abs(loss) or cosine(npy(d0), npy(d_audio)) < 0.9999


# ---------------------------------------------------------------------------- true widths, production row count: torch fp32 reference
def _torch_layer_ref(cfg, wL, lo, rank, alpha, p, seed, offset, x, att, lab):
    """transformers' Qwen3 (fp32, on the device) with adapters hooked in as peft's training-mode LoraLayer: masks materialised
    by ta_lora_dropout_keep."""
    from transformers import Qwen3Config, Qwen3ForCausalLM
    c = Qwen3Config(vocab_size=cfg["vocab"], hidden_size=cfg["hidden"], intermediate_size=cfg["ffn"], num_hidden_layers=cfg["layers"],
                    num_attention_heads=cfg["heads"], num_key_value_heads=cfg["kv_heads"], head_dim=cfg["head_dim"],
                    rms_norm_eps=cfg["rms_eps"], tie_word_embeddings=True,
                    rope_parameters={"rope_theta": cfg["rope_theta"], "rope_type": "default"},
                    max_position_embeddings=4096, attention_bias=False, use_cache=False)
    c._attn_implementation = "eager"
    m = Qwen3ForCausalLM(c).float().eval()
    sd = {k: torch.from_numpy(v) for k, v in wL.items()}
    sd["lm_head.weight"] = sd["model.embed_tokens.weight"]
    m.load_state_dict(sd, strict=False)
    m.tie_weights()
    m = m.to(DEV).requires_grad_(False)
    B, L, _ = x.shape
    s = float(alpha) / rank
    lt = {k: torch.from_numpy(v).to(DEV).requires_grad_(True) for k, v in lo.items()}
    hooks = []
    for name, mod in m.named_modules():
        if isinstance(mod, torch.nn.Linear) and f"{name}.lora_A" in lt:
            layer = int(name.split("layers.")[1].split(".")[0])
            j = LD.PEFT_ORDER.index(name.rsplit(".", 1)[1])
            keep = torch.from_numpy(device_keep(p, seed, offset, layer, j, B * L, mod.in_features)).to(DEV).float()
            A, Bm, sc = lt[f"{name}.lora_A"], lt[f"{name}.lora_B"], float(LD.inv_keep(p))

            def hook(mod_, inp, out, A=A, Bm=Bm, keep=keep, sc=sc):
                xin = inp[0].reshape(B * L, -1)
                return out + (s * (((xin * keep * sc) @ A.t()) @ Bm.t())).reshape(out.shape)
            hooks.append(mod.register_forward_hook(hook))
    xt = torch.from_numpy(x).to(DEV).requires_grad_(True)
    out = m(inputs_embeds=xt, attention_mask=torch.from_numpy(att).to(DEV), labels=torch.from_numpy(lab).to(DEV))
    out.loss.backward()
    return float(out.loss.detach()), npy(xt.grad), {k: npy(v.grad) for k, v in lt.items()}


@pytest.mark.timeout(900)
def test_lora_dropout_true_width_vs_torch():
    """Qwen3-0.6B widths (hidden 1024, ffn 3072, 16 / 8 heads), one layer, B * L = 6144 rows (the skinny kernels' production NCB / RB
    variants and row chunking): masked xa (loss), masked dA (adapter gradients) and the masked d(x) term (d inputs_embeds) against
    torch fp32 with the same masks."""
    cfg = OW.lm_config(vocab=2048, layers=1)
    wL = OW.init_lm(cfg, 1)
    lo = _adapters(cfg, 8, None)
    p, seed, offset = 0.1, 77, 1 << 33
    rng = np.random.RandomState(3)
    B, L = 32, 192
    x = (rng.standard_normal((B, L, cfg["hidden"])) / np.sqrt(cfg["hidden"])).astype(np.float32)
    att = np.ones((B, L), np.int64); att[5, 150:] = 0
    lab = np.full((B, L), -100, np.int64); lab[:, 120:191] = rng.randint(0, 2000, (B, 71))
    lm = _lm(cfg, 8, 32, None, p, lo, wL)
    loss, d_audio, lg = _run(lm, x, att, lab, (p, seed, offset))
    rl, rdx, rg = _torch_layer_ref(cfg, wL, lo, 8, 32, p, seed, offset, x, att, lab)
    assert abs(loss - rl) < 5e-3 * rl, (loss, rl)
    valid = att.astype(bool)
    assert cosine(npy(d_audio).reshape(x.shape)[valid], rdx[valid]) > 0.999
    got = _grads_by_name(lm, lg)
    for k in lo:
        assert cosine(got[k], rg[k]) > 0.998, k


# ---------------------------------------------------------------------------- reproducibility, eval / decoding untouched
def test_lora_dropout_reproducible_and_eval_untouched():
    cfg = R.SMALL["lm"]
    wL, lo = OW.init_lm(cfg, seed=1), _adapters(cfg, 8, None)
    x, att, lab = R.lm_input()
    lm = _lm(cfg, 8, 32, None, 0.1, lo, wL)
    _, d1, g1 = _run(lm, x, att, lab, (0.1, 5, 9))
    _, d2, g2 = _run(lm, x, att, lab, (0.1, 5, 9))
    for a, b in zip(g1, g2):
        assert torch.equal(a, b)                              # same descriptor: the same bits
    assert torch.equal(d1, d2)
    _, _, g3 = _run(lm, x, att, lab, (0.1, 5, 10))
    assert not all(torch.equal(a, b) for a, b in zip(g1, g3))  # another offset: other masks
    # evaluation: FrozenLMLoss of an eval() model with p = 0.1 equals the p = 0 model bit for bit; the offset does not move
    lm0 = _lm(cfg, 8, 32, None, 0.0, lo, wL)
    B, L, D = x.shape
    ids = torch.full((B, L), cfg["vocab"] - 1, dtype=torch.int64, device=DEV)
    src = torch.arange(B * L, dtype=torch.int32, device=DEV)
    rows, tg, n = ops.label_rows(torch.from_numpy(lab).to(DEV))
    n = int(n.item())
    audio = torch.from_numpy(x.reshape(B * L, D)).to(DEV)
    kmask = torch.from_numpy(att).to(DEV).int()
    lm.eval(); lm0.eval()
    off = lm.lora_drop_offset
    a = FrozenLMLoss.apply(audio, lm, ids, src, kmask, rows, tg, n, 1.0 / n, True, *lm.lora_parameters())
    b = FrozenLMLoss.apply(audio, lm0, ids, src, kmask, rows, tg, n, 1.0 / n, True, *lm0.lora_parameters())
    assert lm.lora_drop_offset == off
    assert torch.equal(a[2], b[2]) and torch.equal(a[1], b[1])
    # training mode draws a fresh offset per forward and changes the logits
    lm.train()
    c_ = FrozenLMLoss.apply(audio, lm, ids, src, kmask, rows, tg, n, 1.0 / n, True, *lm.lora_parameters())
    assert lm.lora_drop_offset == off + 1 and not torch.equal(c_[2], b[2])
    # decoding: identical tokens for p = 0.1 (even in train mode) and p = 0
    am = torch.from_numpy(att[:, :40]).to(DEV)
    t1 = lm.greedy_decode(ids[:, :40], src.view(B, L)[:, :40].reshape(-1).contiguous(), audio, am, max_new_tokens=6)
    t0 = lm0.greedy_decode(ids[:, :40], src.view(B, L)[:, :40].reshape(-1).contiguous(), audio, am, max_new_tokens=6)
    assert torch.equal(t1, t0)


def _op_inputs(cfg, packed):
    """-> (ids, src_row, audio f32 [B*L, D], kmask, label rows, label targets, n, pos, seg): the rows of ``R.lm_input()`` or -- ``packed`` --
    the smallest packed batch tests/test_gpu_packing.py builds (two clips in one row, one clip in the other), inputs_embeds fed as
    <audio> rows."""
    if packed:
        from tests.test_gpu_packing import packed_batch
        x, sid, lab, _ = packed_batch([[40, 56], [96]], cfg["hidden"], cfg["vocab"])
        s = torch.from_numpy(sid).to(DEV)
        kmask = (s != 0).int().contiguous()
        seg, pos = ops.segment_table(s)
    else:
        x, att, lab = R.lm_input()
        kmask, seg, pos = torch.from_numpy(att).to(DEV).int(), None, None
    B, L, D = x.shape
    ids = torch.full((B, L), cfg["vocab"] - 1, dtype=torch.int64, device=DEV)
    src = torch.arange(B * L, dtype=torch.int32, device=DEV)
    rows, tg, n = ops.label_rows(torch.from_numpy(lab).to(DEV))
    return ids, src, torch.from_numpy(x.reshape(B * L, D)).to(DEV), kmask, rows, tg, int(n.item()), pos, seg


def test_lora_dropout_ops_pass_opcheck():
    """The one LM operator in its three forms: no options, LoRA dropout, a segment table with that dropout."""
    from tiny_audio_amd import torch_ops
    cfg = R.SMALL["lm"]
    lm = _lm(cfg, 8, 32, None, 0.1, _adapters(cfg, 8, None), OW.init_lm(cfg, seed=1))
    utils = ("test_schema", "test_faketensor", "test_autograd_registration")
    for packed, options in ((False, ()), (False, (None, 0.1, 12345, 3)), (True, (0.1, 12345, 3))):
        ids, src, audio, kmask, rows, tg, n, pos, seg = _op_inputs(cfg, packed)
        args = (audio.requires_grad_(True), list(lm.lora_parameters()), torch_ops.register_module(lm), ids, src, kmask, rows, tg, n, 1.0 / n,
                False, pos, *((seg,) if packed else ()), *options)
        torch.library.opcheck(torch.ops.ta355.lm_forward_loss, args, test_utils=utils)


@pytest.mark.parametrize("drop", [None, (0.1, 777, 5)], ids=["nodrop", "drop"])
@pytest.mark.parametrize("packed", [False, True], ids=["rows", "packed"])
def test_operator_route_equals_the_direct_calls_bit_for_bit(packed, drop):
    """``FrozenLMLoss.apply`` + ``loss.backward()`` (the custom-operator pair and its autograd node) against ``forward_loss`` /
    ``backward_from_ctx`` handed the same table and the same (p, seed, offset): both routes issue the same launches with the same
    arguments and d(loss) is exactly 1, so every result is the same bits (a repeated descriptor reproduces them:
    test_lora_dropout_reproducible_and_eval_untouched)."""
    cfg = R.SMALL["lm"]
    lm = _lm(cfg, 8, 32, None, drop[0] if drop else 0.0, _adapters(cfg, 8, None), OW.init_lm(cfg, seed=1))
    ids, src, audio, kmask, rows, tg, n, pos, seg = _op_inputs(cfg, packed)
    loss, nll, logits, ctx = lm.forward_loss(ids, src, audio, kmask, rows, tg, n, 1.0 / n, want_logits=True, pos=pos, lora_dropout=drop, seg=seg)
    d_audio, _, lg = lm.backward_from_ctx(ctx, audio.shape[0])
    lm.train()
    if drop:
        lm.lora_drop_seed, lm.lora_drop_offset = drop[1], drop[2]
    a = audio.clone().requires_grad_(True)
    params = lm.lora_parameters()
    o_loss, o_nll, o_logits = FrozenLMLoss.apply(a, lm, ids, src, kmask, rows, tg, n, 1.0 / n, True, *params, pos=pos, seg=seg)
    o_loss.backward()
    assert lm.lora_drop_offset == (drop[2] + 1 if drop else 0)
    assert torch.equal(o_loss, loss.reshape(())) and torch.equal(o_nll, nll) and torch.equal(o_logits, logits)
    assert torch.equal(a.grad, d_audio)
    assert len(params) == len(lg) == 8
    for p_, g_ in zip(params, lg):
        assert g_.abs().sum() > 0 and torch.equal(p_.grad, g_)


def test_stage2_trains_with_lora_dropout():
    """ASRTrainer, stage 2 (frozen projector, adapters on all 7 linears) at p = 0.1 with the LM in training mode: every step draws
    fresh masks; finite, decreasing loss."""
    from tests.test_gpu_parity import build_model
    from tiny_audio_amd.trainer import ASRTrainer, TrainingArguments
    S = R.SMALL
    wE, wL = OW.init_encoder(S["enc"], 0), OW.init_lm(S["lm"], 1)
    wP = OW.init_mlp_projector(S["enc"]["hidden"], S["lm"]["hidden"], S["proj_hidden"])
    m = build_model(S["enc"], S["lm"], S["proj_hidden"], wE, wL, wP, audio_token_id=S["audio_token_id"], audio_token_dropout=0.0,
                    use_lora=True, freeze_projector=True, lora_dropout=0.1)
    assert m.language_model.lora_dropout == 0.1
    feats = torch.from_numpy(R.encoder_input())
    B = feats.shape[0]
    counts = np.full(B, m.projector.get_output_length(m.audio_tower.output_length(feats.shape[2])), np.int64)
    ids, att, lab, counts = R.asr_tokens(counts)
    tb = dict(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(att), labels=torch.from_numpy(lab),
              audio_token_counts=torch.from_numpy(counts))
    tr = ASRTrainer(m, TrainingArguments(learning_rate=2e-3, warmup_steps=0, max_steps=10, lr_scheduler_type="constant", weight_decay=0.0))
    m.train()
    m.language_model.train(True)                      # ASRModel.train() keeps the frozen LM (and peft's dropout) in eval mode
    off = m.language_model.lora_drop_offset
    losses = [float(tr.training_step(dict(input_features=feats, **tb))) for _ in range(10)]
    assert all(np.isfinite(losses)), losses
    assert m.language_model.lora_drop_offset == off + 10
    assert np.mean(losses[-3:]) < losses[0] - 0.05, losses

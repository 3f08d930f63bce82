"""SmolLM3 / Llama-style text tower on the device (no q_norm / k_norm, per-layer NoPE) against transformers' own ``SmolLM3ForCausalLM`` /
``LlamaForCausalLM`` in fp32 on the CPU, built from a small random config here; weights are rebuilt from a seed (oracle.weights.init_lm
minus the norm keys), never stored.  Gates are the project's existing ones for the same quantities (tests/test_gpu_round2.py:283-289:
loss within 5e-3 relative, logits max-abs < 0.1 and RMS < 0.02, gradient cosine > 0.999; adapter gradients > 0.998,
tests/test_gpu_parity.py:355; greedy near-tie tolerance 0.12 with at least 26 of 32 decisions exact, tests/test_gpu_parity.py:548-578,645).

Measured on an MI355X (this file's own prints, max over the cases of each test; transformers' own bf16 run of the same model on the
CPU against its fp32 run in brackets) -- see profiles/smollm3.md for the table."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import weights as OW

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tiny_audio_amd import _lib, ops
    from tiny_audio_amd.asr_config import ASRConfig, LMConfig
    from tiny_audio_amd.language_model import Qwen3MI355X
    from tiny_audio_amd.ops import ptr, stream

DEV = "cuda"
V, D, F = 1000, 512, 768
AUDIO_ID = V - 1
THETA = 2e6


def cosine(a, b):
    a = np.asarray(a, np.float64).ravel(); b = np.asarray(b, np.float64).ravel()
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-30))


def npy(t):
    return t.detach().float().cpu().numpy()


def logit_err(got, ref):
    d = np.asarray(got, np.float64) - np.asarray(ref, np.float64)
    return float(np.abs(d).max()), float(np.sqrt((d ** 2).mean()))


def logits_close(got, ref):
    mx, rms = logit_err(got, ref)
    return mx < 0.1 and rms < 0.02


# ----------------------------------------------------------------------------- the transformers reference
def tower(kind="smollm3", heads=4, kv=1, layers=4, hidden=D, ffn=F, vocab=V, seed=1, no_rope_layers=None, embed_scale=1.0, max_pos=512):
    """-> (transformers model in fp32 on the CPU, its state dict as numpy, the LMConfig source dict)."""
    import transformers
    geom = dict(vocab_size=vocab, hidden_size=hidden, intermediate_size=ffn, num_hidden_layers=layers, num_attention_heads=heads,
                num_key_value_heads=kv, max_position_embeddings=max_pos, rms_norm_eps=1e-6, tie_word_embeddings=True,
                rope_parameters=dict(rope_type="default", rope_theta=THETA), pad_token_id=None, bos_token_id=1, eos_token_id=2)
    if kind == "smollm3":
        cfg = transformers.SmolLM3Config(**geom, no_rope_layers=no_rope_layers)
        model = transformers.SmolLM3ForCausalLM(cfg)
    else:
        cfg = transformers.LlamaConfig(**geom, attention_bias=False, mlp_bias=False)
        model = transformers.LlamaForCausalLM(cfg)
    w = OW.init_lm(OW.lm_config(vocab, hidden, ffn, layers, heads, kv, hidden // heads, 1e-6, THETA), seed)
    w = {k: v for k, v in w.items() if "q_norm" not in k and "k_norm" not in k}
    w["model.embed_tokens.weight"] = (w["model.embed_tokens.weight"] * embed_scale).astype(np.float32)
    res = model.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=False)
    assert not res.unexpected_keys and set(res.missing_keys) <= {"lm_head.weight"}, res
    model.tie_weights()
    assert model.lm_head.weight.data_ptr() == model.model.embed_tokens.weight.data_ptr()
    model = model.float().eval()
    model.config._attn_implementation = "eager"
    return model, w, cfg.to_dict()


def hip_lm(w, src, res_f32=False, **over):
    lm = Qwen3MI355X(LMConfig(dict(src, **over)), DEV)
    lm.res_f32 = res_f32
    return lm.load_state_dict_hf(w)


def hf_run(model, x, att, pos, lab, dtype=torch.float32):
    """-> loss, logits [B, L, V], d(loss)/d(inputs_embeds) of the transformers model (sum-CE over the shifted labels / n)."""
    m = model if dtype == torch.float32 else model.to(dtype)
    xe = torch.from_numpy(x).to(dtype).requires_grad_(True)
    out = m(inputs_embeds=xe, attention_mask=torch.from_numpy(att), position_ids=torch.from_numpy(pos).long(), use_cache=False)
    logits = out.logits.float()
    tl = torch.from_numpy(lab)[:, 1:].reshape(-1)
    n = int((tl != -100).sum())
    loss = torch.nn.functional.cross_entropy(logits[:, :-1].reshape(-1, logits.shape[-1]), tl, ignore_index=-100, reduction="sum") / n
    loss.backward()
    if dtype != torch.float32:
        model.float()
    return float(loss.detach()), logits.detach().numpy(), xe.grad.float().numpy(), n


def hip_run(lm, x, att, pos, lab, lora=False):
    """The same through ta_lm_forward_loss / ta_lm_backward, the inputs_embeds fed as <audio> rows."""
    B, L, Dm = x.shape
    ids = torch.full((B, L), lm.config.vocab_size - 1, dtype=torch.int64, device=DEV)
    src = torch.arange(B * L, dtype=torch.int32, device=DEV)
    rows, tg, n = ops.label_rows(torch.from_numpy(lab).to(DEV))
    n = int(n.item())
    loss, nll, logits, ctx = lm.forward_loss(ids, src, torch.from_numpy(x.reshape(B * L, Dm)).to(DEV), torch.from_numpy(att).to(DEV).int(),
                                             rows, tg, n, 1.0 / n, want_logits=True, pos=torch.from_numpy(pos).to(DEV).int().reshape(-1).contiguous(),
                                             lora_dropout=lm.next_lora_dropout())
    d_audio, _, lg = lm.backward_from_ctx(ctx, B * L)
    torch.cuda.synchronize()
    return float(loss), npy(logits).reshape(B, L, -1)[:, :, :lm.config.vocab_size], npy(d_audio).reshape(B, L, Dm), n, lg


def ragged_batch(B, L, hidden=D, vocab=V, seed=3):
    """inputs_embeds, a right-padded clip 0 and (B > 1) a left-padded clip 1, explicit position ids, labels on the tail of every clip."""
    rng = np.random.RandomState(seed)
    x = rng.standard_normal((B, L, hidden)).astype(np.float32)
    att = np.ones((B, L), np.int64)
    att[0, L - L // 8:] = 0
    if B > 1:
        att[1, :L // 10] = 0
    pos = np.clip(np.cumsum(att, -1) - 1, 0, None).astype(np.int64)
    lab = np.full((B, L), -100, np.int64)
    tok = rng.randint(0, vocab - 1, (B, L))
    lab[0, L // 3:L - L // 8] = tok[0, L // 3:L - L // 8]
    if B > 1:
        lab[1:, L // 2:] = tok[1:, L // 2:]
    return x, att, pos, lab


def check_case(model, lm, x, att, pos, lab, tag):
    rl, rlog, rdx, rn = hf_run(model, x, att, pos, lab)
    gl, glog, gdx, gn, _ = hip_run(lm, x, att, pos, lab)
    valid = att.astype(bool)
    mx, rms = logit_err(glog[valid], rlog[valid])
    cs = cosine(gdx[valid], rdx[valid])
    print(f"[smollm3] {tag}: loss {gl:.5f} vs {rl:.5f} (rel {abs(gl - rl) / rl:.2e}), logits max {mx:.4f} rms {rms:.4f}, d(audio) cosine {cs:.6f}")
    assert gn == rn
    assert abs(gl - rl) < 5e-3 * rl, tag
    assert mx < 0.1 and rms < 0.02, tag
    assert cs > 0.999, tag
    return rlog


# ============================================================================ 1. small tower, both attention paths, both stream modes
@pytest.mark.parametrize("res_f32", [False, True], ids=["bf16stream", "f32stream"])
@pytest.mark.parametrize("heads,kv", [(4, 1), (4, 2)], ids=["group4", "group2"])
@pytest.mark.parametrize("L", [80, 200], ids=["fused", "twokernel"])
def test_small_tower_vs_transformers(L, heads, kv, res_f32):
    """4 layers, layer 3 NoPE; L = 80 lies inside the fused envelope of both groups (4 * ceil(80 / 32) = 12), L = 200 outside it."""
    model, w, src = tower("smollm3", heads, kv)
    assert src["no_rope_layers"] == [1, 1, 1, 0]
    lm = hip_lm(w, src, res_f32)
    assert lm._w.nope_layers == 0b1000 and lm._layers_arr[0].qn_w is None
    x, att, pos, lab = ragged_batch(2, L)
    check_case(model, lm, x, att, pos, lab, f"L={L} {heads}/{kv} res_f32={res_f32}")


def test_small_tower_bf16_reference_of_transformers():
    """Not a gate on this project's code: transformers' OWN bf16 run of the same model against its fp32 run, printed beside the numbers
    above for profiles/smollm3.md (how much of the distance is the number format)."""
    model, w, src = tower("smollm3", 4, 1)
    x, att, pos, lab = ragged_batch(2, 80)
    rl, rlog, rdx, _ = hf_run(model, x, att, pos, lab)
    bl, blog, bdx, _ = hf_run(model, x, att, pos, lab, dtype=torch.bfloat16)
    valid = att.astype(bool)
    mx, rms = logit_err(blog[valid], rlog[valid])
    print(f"[smollm3] transformers bf16 vs fp32: loss rel {abs(bl - rl) / rl:.2e}, logits max {mx:.4f} rms {rms:.4f}, d(embeds) cosine {cosine(bdx[valid], rdx[valid]):.6f}")
    assert np.isfinite(bl)


# ============================================================================ 2. the two switches are independent
@pytest.mark.parametrize("L", [80, 200], ids=["fused", "twokernel"])
def test_llama_tower_no_norm_all_rope(L):
    model, w, src = tower("llama", 4, 2, layers=3)
    lm = hip_lm(w, src)
    assert lm._w.nope_layers == 0 and lm._layers_arr[0].qn_w is None and lm.config.model_type == "llama"
    x, att, pos, lab = ragged_batch(2, L)
    check_case(model, lm, x, att, pos, lab, f"llama L={L}")


@pytest.mark.parametrize("L", [80, 200], ids=["fused", "twokernel"])
def test_nope_flag_is_read_by_the_training_paths(L):
    """The SmolLM3 weights with the NoPE flag cleared (every layer rotating) must MISS the logits gate against the SmolLM3 reference."""
    model, w, src = tower("smollm3", 4, 1, no_rope_layers=[1, 0, 1, 0])
    x, att, pos, lab = ragged_batch(2, L)
    rlog = check_case(model, hip_lm(w, src), x, att, pos, lab, f"nope [1,0,1,0] L={L}")
    wrong = hip_lm(w, src, no_rope_layers=[1, 1, 1, 1])
    assert wrong._w.nope_layers == 0
    _, glog, _, _, _ = hip_run(wrong, x, att, pos, lab)
    valid = att.astype(bool)
    mx, rms = logit_err(glog[valid], rlog[valid])
    print(f"[smollm3] flag cleared L={L}: logits max {mx:.4f} rms {rms:.4f}")
    assert not (mx < 0.1 and rms < 0.02)


# ============================================================================ 3. decoding
def cache_logits(lm, x, att, forced, nope_layers=None):
    """ta_lm_prefill over the prompt (inputs_embeds x [B, L, D] as <audio> rows), then one ta_lm_decode_step per column of ``forced``
    [B, T]: -> f32 logits [T + 1, B, V] (row 0: after the prompt; row t + 1: after forced[:, t]).  The host does ta_greedy_advance's
    bookkeeping (position, slot, key mask) so that the tokens can be forced.  ``nope_layers``: override the handle's flag."""
    L_ = _lib.lib()
    c = lm.config
    B, L, Dm = x.shape
    T = forced.shape[1]
    Lmax = L + T
    w = lm._w
    if nope_layers is not None:
        w = _lib.LmWeights.from_buffer_copy(lm._w)
        w.nope_layers = nope_layers
    i32 = torch.int32
    a = torch.from_numpy(att).to(DEV).to(i32).contiguous()
    kmask = torch.zeros((B, Lmax), dtype=i32, device=DEV); kmask[:, :L] = a
    pos_full = (a.cumsum(-1) - 1).clamp(min=0).to(i32).contiguous()
    n_valid = a.sum(-1).to(i32)
    last = (torch.arange(L, device=DEV, dtype=i32)[None] * a).max(-1).values
    last_rows = (torch.arange(B, device=DEV, dtype=i32) * L + last.to(i32)).contiguous()
    shape = (c.num_hidden_layers, B, c.num_key_value_heads, Lmax, c.head_dim)
    kc, vc = torch.zeros(shape, dtype=torch.bfloat16, device=DEV), torch.zeros(shape, dtype=torch.bfloat16, device=DEV)
    ws = torch.empty(max(L_.ta_lm_prefill_workspace_bytes(C.byref(w), B, L), L_.ta_lm_decode_workspace_bytes(C.byref(w), B)), dtype=torch.uint8, device=DEV)
    logits = torch.empty((B, lm.vocab_pad), dtype=torch.float32, device=DEV)
    ids = torch.full((B, L), c.vocab_size - 1, dtype=torch.int64, device=DEV)
    src = torch.arange(B * L, dtype=i32, device=DEV)
    audio = torch.from_numpy(x.reshape(B * L, Dm)).to(DEV)
    _lib.check(L_.ta_lm_prefill(C.byref(w), ptr(ids), ptr(src), ptr(audio), ptr(a), ptr(pos_full), B, L, ptr(kc), ptr(vc), Lmax, ptr(last_rows),
                                ptr(logits), None, ptr(ws), ws.numel(), stream()), "ta_lm_prefill")
    out = [logits[:, :c.vocab_size].clone()]
    for t in range(T):
        nxt = torch.from_numpy(np.ascontiguousarray(forced[:, t])).to(DEV)
        pos = (n_valid + t).to(i32).contiguous()
        slot = torch.full((1,), L + t, dtype=i32, device=DEV)
        kmask[:, L + t] = 1
        _lib.check(L_.ta_lm_decode_step(C.byref(w), ptr(nxt), ptr(pos), ptr(kmask), ptr(slot), B, ptr(kc), ptr(vc), Lmax, ptr(logits), None,
                                        ptr(ws), ws.numel(), stream()), "ta_lm_decode_step")
        out.append(logits[:, :c.vocab_size].clone())
    torch.cuda.synchronize()
    return npy(torch.stack(out))


def hf_step_logits(model, w, x, att, tokens):
    """fp32 logits [T + 1, B, V] of the transformers model after the prompt and after every token of ``tokens`` [B, T] (one causal pass
    over prompt + tokens; the prompt may be right-padded: the new tokens follow the padding, as in the KV cache)."""
    B, L, _ = x.shape
    T = tokens.shape[1]
    emb = w["model.embed_tokens.weight"]
    xe = np.concatenate([x, emb[tokens]], axis=1)
    am = np.concatenate([att, np.ones((B, T), np.int64)], axis=1)
    pos = np.clip(np.cumsum(am, -1) - 1, 0, None)
    with torch.no_grad():
        lg = model(inputs_embeds=torch.from_numpy(xe), attention_mask=torch.from_numpy(am), position_ids=torch.from_numpy(pos), use_cache=False).logits.numpy()
    last = (np.arange(L)[None] * att).max(-1)
    return np.stack([lg[np.arange(B), last]] + [lg[:, L + t] for t in range(T)])


def _set_decode_fused(on):
    os.environ["TA355_DECODE_FUSED"] = "1" if on else "0"
    _lib.lib().ta_gemm_reload_knobs()


def _decode_case():
    model, w, src = tower("smollm3", 4, 1)
    rng = np.random.RandomState(11)
    B, L = 2, 40
    x = rng.standard_normal((B, L, D)).astype(np.float32)
    att = np.ones((B, L), np.int64); att[1, 33:] = 0
    return model, w, src, x, att


def test_greedy_decoding_vs_transformers_and_fused_vs_unfused():
    """2 clips x 16 tokens, judged step by step on the HIP path's own prefix by the transformers model's fp32 logits with the near-tie rule
    of tests/test_gpu_parity.py:_check_greedy_against_oracle (tol 0.12, at least 26 of 32 decisions exact); the fused and the round-3
    decode sequences emit the same tokens."""
    model, w, src, x, att = _decode_case()
    lm = hip_lm(w, src)
    B, L, _ = x.shape
    max_new = 16
    assert max_new > 1                                   # generated positions enter the NoPE layer's cache beyond the prompt
    ids = torch.full((B, L), V - 1, dtype=torch.int64, device=DEV)
    srcr = torch.arange(B * L, dtype=torch.int32, device=DEV)
    audio = torch.from_numpy(x.reshape(B * L, D)).to(DEV)
    am = torch.from_numpy(att).to(DEV)
    toks = {}
    try:
        for fused in (True, False):
            _set_decode_fused(fused)
            toks[fused] = lm.greedy_decode(ids, srcr, audio, am, max_new_tokens=max_new, eos_ids=(), pad_id=0).cpu().numpy()
    finally:
        _set_decode_fused(True)
    assert toks[True].shape == (B, max_new)
    np.testing.assert_array_equal(toks[True], toks[False])
    ref = hf_step_logits(model, w, x, att, toks[True])
    exact, worst = 0, 0.0
    for t in range(max_new):
        for b in range(B):
            gap = float(ref[t, b].max() - ref[t, b, toks[True][b, t]])
            worst = max(worst, gap)
            assert gap < 0.12, (b, t, int(toks[True][b, t]), int(ref[t, b].argmax()))
            exact += int(toks[True][b, t] == ref[t, b].argmax())
    print(f"[smollm3] greedy: {exact} of {B * max_new} decisions exact, worst gap to the reference argmax {worst:.4f}")
    assert exact >= 26


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "round3"])
def test_kv_cache_logits_vs_transformers_and_training_path(fused):
    """Teacher-forced: prefill + 6 decode steps against (a) transformers fp32 and (b) this library's own training-path forward over prompt
    + tokens; and with the handle's NoPE flag cleared the same logits must MISS the gate (prefill: row 0; decode: the later rows)."""
    model, w, src, x, att = _decode_case()
    lm = hip_lm(w, src)
    B, L, _ = x.shape
    T = 6
    forced = np.random.RandomState(5).randint(0, V - 1, (B, T)).astype(np.int64)
    ref = hf_step_logits(model, w, x, att, forced)
    try:
        _set_decode_fused(fused)
        got = cache_logits(lm, x, att, forced)
        wrong = cache_logits(lm, x, att, forced, nope_layers=0)
    finally:
        _set_decode_fused(True)
    mx, rms = logit_err(got, ref)
    print(f"[smollm3] kv-cache logits ({'fused' if fused else 'round-3'} decode): max {mx:.4f} rms {rms:.4f}")
    assert mx < 0.1 and rms < 0.02
    # (b) the training path over prompt + tokens
    emb = w["model.embed_tokens.weight"]
    xe = np.concatenate([x, emb[forced]], axis=1).astype(np.float32)
    am = np.concatenate([att, np.ones((B, T), np.int64)], axis=1)
    pos = np.clip(np.cumsum(am, -1) - 1, 0, None)
    lab = np.full(am.shape, -100, np.int64); lab[:, L:] = forced
    _, tlog, _, _, _ = hip_run(lm, xe, am, pos, lab)
    last = (np.arange(L)[None] * att).max(-1)
    train = np.stack([tlog[np.arange(B), last]] + [tlog[:, L + t] for t in range(T)])
    mx2, rms2 = logit_err(got, train)
    print(f"[smollm3] kv-cache vs training path: max {mx2:.4f} rms {rms2:.4f}")
    assert mx2 < 0.1 and rms2 < 0.02
    # the flag is read by prefill (row 0 depends on nothing else) and by the decode step (rows 1..)
    for name, sl in (("prefill", slice(0, 1)), ("decode", slice(1, None))):
        wm, wr = logit_err(wrong[sl], ref[sl])
        print(f"[smollm3] flag cleared, {name}: max {wm:.4f} rms {wr:.4f}")
        assert not (wm < 0.1 and wr < 0.02), name


# ============================================================================ 4. LoRA
LORA_TARGETS = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")


def test_lora_rank8_all_targets_vs_functional_call():
    """Reference: the transformers model through torch.func.functional_call with every targeted weight replaced by W + (alpha / r) B A built
    from leaf tensors, so autograd yields dA and dB."""
    model, w, src = tower("smollm3", 4, 1)
    r, alpha = 8, 32
    lo = OW.init_lora(OW.lm_config(V, D, F, 4, 4, 1, 128, 1e-6, THETA), rank=r, seed=4)
    lm = hip_lm(w, src)
    lm.enable_lora(rank=r, alpha=alpha).load_lora_state_dict(lo)
    x, att, pos, lab = ragged_batch(2, 80)
    leaves = {k: torch.from_numpy(v).clone().requires_grad_(True) for k, v in lo.items()}
    params = {k: v for k, v in model.named_parameters()}
    rep = dict(params)
    for i in range(4):
        for t in LORA_TARGETS:
            k = f"model.layers.{i}.{t}"
            rep[k + ".weight"] = params[k + ".weight"].detach() + (alpha / r) * leaves[k + ".lora_B"] @ leaves[k + ".lora_A"]
    rep["lm_head.weight"] = rep["model.embed_tokens.weight"]
    xe = torch.from_numpy(x)
    out = torch.func.functional_call(model, rep, args=(), kwargs=dict(inputs_embeds=xe, attention_mask=torch.from_numpy(att),
                                                                       position_ids=torch.from_numpy(pos), use_cache=False))
    logits = out.logits
    tl = torch.from_numpy(lab)[:, 1:].reshape(-1)
    n = int((tl != -100).sum())
    rl = torch.nn.functional.cross_entropy(logits[:, :-1].reshape(-1, V), tl, ignore_index=-100, reduction="sum") / n
    rl.backward()
    rl = rl.detach()
    gl, glog, gdx, gn, lg = hip_run(lm, x, att, pos, lab)
    assert gn == n and abs(gl - float(rl)) < 5e-3 * float(rl)
    valid = att.astype(bool)
    assert logits_close(glog[valid], logits.detach().numpy()[valid])
    base = hf_run(model, x, att, pos, lab)[1]
    assert np.abs(base[valid] - logits.detach().numpy()[valid]).max() > 0.3        # the adapters matter in this case
    for p_, g_ in zip(lm.lora_parameters(), lg):
        p_.data.copy_(g_)
    got = lm.export_lora_state_dict(prefix="model.", suffix="")
    assert set(got) == set(leaves)
    worst = min(cosine(npy(got[k]), leaves[k].grad.numpy()) for k in leaves)
    print(f"[smollm3] lora: loss {gl:.5f} vs {float(rl):.5f}, worst adapter-gradient cosine {worst:.6f}")
    for k in leaves:
        assert cosine(npy(got[k]), leaves[k].grad.numpy()) > 0.998, k


def test_lora_dropout_runs_and_is_reproducible():
    model, w, src = tower("smollm3", 4, 1)
    lo = OW.init_lora(OW.lm_config(V, D, F, 4, 4, 1, 128, 1e-6, THETA), rank=8, seed=4)
    x, att, pos, lab = ragged_batch(2, 80)
    runs = []
    for _ in range(2):
        lm = hip_lm(w, src)
        lm.enable_lora(rank=8, alpha=32, dropout=0.1, seed=7).load_lora_state_dict(lo)
        lm.train()
        runs.append(hip_run(lm, x, att, pos, lab))
    lm0 = hip_lm(w, src)
    lm0.enable_lora(rank=8, alpha=32).load_lora_state_dict(lo)
    plain = hip_run(lm0, x, att, pos, lab)
    assert np.isfinite(runs[0][0]) and runs[0][0] == runs[1][0]
    np.testing.assert_array_equal(runs[0][1], runs[1][1])
    assert all(torch.equal(a, b) for a, b in zip(runs[0][4], runs[1][4]))
    assert not np.array_equal(runs[0][1], plain[1])                                 # the masks did something


# ============================================================================ 5. true width
def test_true_width_two_layers_second_nope():
    """SmolLM3-3B widths (D 2048, F 11008, 16 / 4 heads, V 128 257) at depth 2, layer 1 NoPE, B = 1: the GEMM (N = 2F = 22016) and LM-head
    (V_pad = 128384) shapes nothing else reaches."""
    Vt = 128257
    model, w, src = tower("smollm3", 16, 4, layers=2, hidden=2048, ffn=11008, vocab=Vt, no_rope_layers=[1, 0], max_pos=256)
    lm = hip_lm(w, src)
    assert lm.vocab_pad == 128384 and lm._w.nope_layers == 0b10
    x, att, pos, lab = ragged_batch(1, 48, hidden=2048, vocab=Vt, seed=9)
    check_case(model, lm, x, att, pos, lab, "true width")


# ============================================================================ 6. full fine-tuning is refused, in words
def test_full_finetune_raises_the_documented_error():
    from tiny_audio_amd.asr_modeling import ASRModel
    _, w, src = tower("smollm3", 4, 1)
    enc = OW.enc_config(hidden=256, ffn=512, layers=1, heads=4)
    with pytest.raises(NotImplementedError, match="q/k-norm"):
        ASRModel(ASRConfig(audio_config=enc, text_config=src, projector_hidden_dim=128, audio_token_id=999, pad_token_id=990, eos_token_id=991,
                           freeze_language_model=False), device=DEV, init="none")
    with pytest.raises(NotImplementedError, match="q/k-norm"):
        hip_lm(w, src).enable_full_finetune()

"""-m gpu: the Whisper audio tower (80 / 128 mel bins, 30 s window) on the HIP path against transformers.

Yardsticks: the fixtures tests/golden/make_whisper_fixture.py wrote from transformers on the CPU (a random-weight WhisperEncoder at
d_model 128 and WhisperFeatureExtractor(feature_size=80), both on the clips of tests/golden/whisper_recipe.py), and transformers built
live on the CPU at whisper-tiny and large-v3 widths.  Gates are the project's own: encoder output rel-to-max error < 2e-2 and
cosine > 0.9995 against the fp32 output (tests/test_gpu_parity.py), log-mel max |diff| < 5e-4 (tests/test_gpu_kernels.py).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import weights as OW
from tests.golden import recipe as R
from tests.golden import whisper_recipe as WR

if torch.cuda.is_available():
    from tiny_audio_amd import torch_ops
    from tiny_audio_amd.asr_config import ASRConfig, WhisperEncoderConfig, compute_encoder_output_length
    from tiny_audio_amd.asr_modeling import ASRModel
    from tiny_audio_amd.asr_processing import ASRProcessor, LogMelFeatureExtractor
    from tiny_audio_amd.trainer import ASRTrainer, TrainingArguments
    from tiny_audio_amd.whisper_encoder import WhisperEncoderMI355X

DEV = "cuda"


def relmax(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))


def cosine(a, b):
    a = np.asarray(a, np.float64).ravel(); b = np.asarray(b, np.float64).ravel()
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-30))


def npy(t):
    return t.detach().float().cpu().numpy()


def small_fixture(golden):
    x = golden("whisper_logmel80.npz")["input_features"]
    ref = np.stack([golden(f"whisper_encoder_small_f32_{b}.npz")["last_hidden_state"] for b in range(2)])
    bits = golden("whisper_encoder_small_bf16.npz")["last_hidden_state_bf16_bits"]
    ref_bf16 = (bits.astype(np.uint32) << 16).view(np.float32)
    return x, ref, ref_bf16


def small_encoder(**kw):
    return WhisperEncoderMI355X(WhisperEncoderConfig(WR.SMALL), DEV).load_state_dict_hf(WR.encoder_weights(**kw))


# ---------------------------------------------------------------------------- (1) the committed fixture
@pytest.mark.parametrize("res_f32", [False, True], ids=["bf16-stream", "fp32-stream"])
def test_encoder_vs_transformers_fixture(golden, res_f32):
    x, ref, ref_bf16 = small_fixture(golden)
    enc = small_encoder()
    enc.res_f32 = res_f32
    out = npy(enc(torch.from_numpy(x), return_f32=True).last_hidden_state)
    assert out.shape == ref.shape == (2, 1500, 128)
    print(f"whisper small fixture res_f32={res_f32}: ours relmax {relmax(out, ref):.5f} cosine {cosine(out, ref):.6f}; "
          f"transformers bf16 module relmax {relmax(ref_bf16, ref):.5f} cosine {cosine(ref_bf16, ref):.6f}")
    assert relmax(out, ref) < 2e-2 and cosine(out, ref) > 0.9995
    out_b = enc(torch.from_numpy(x)).last_hidden_state
    assert out_b.dtype == torch.bfloat16 and relmax(npy(out_b), ref) < 2e-2


def test_position_table_is_applied_row_by_row(golden):
    """A table shifted by one frame, or no table, must NOT pass the gate: the fixture's positions are perturbed so that this shows."""
    x, ref, _ = small_fixture(golden)
    sd = WR.encoder_weights()
    sd["embed_positions.weight"] = np.roll(sd["embed_positions.weight"], 1, axis=0)
    out = npy(WhisperEncoderMI355X(WhisperEncoderConfig(WR.SMALL), DEV).load_state_dict_hf(sd)(torch.from_numpy(x), return_f32=True).last_hidden_state)
    assert relmax(out, ref) > 2e-2


# ---------------------------------------------------------------------------- (2) audio-token dropout
@pytest.mark.parametrize("res_f32", [False, True], ids=["bf16-stream", "fp32-stream"])
def test_frame_keep_zeroes_dropped_frames_without_rescale(golden, res_f32):
    x, _, _ = small_fixture(golden)
    enc = small_encoder()
    enc.res_f32 = res_f32
    full = npy(enc(torch.from_numpy(x), return_f32=True).last_hidden_state)
    keep = (np.random.RandomState(4).rand(2, 1500) < 0.8).astype(np.float32)
    out = npy(enc(torch.from_numpy(x), frame_keep=torch.from_numpy(keep).reshape(-1), return_f32=True).last_hidden_state)
    assert float(np.abs(out[keep == 0]).max()) == 0.0
    assert np.array_equal(out[keep == 1], full[keep == 1])


# ---------------------------------------------------------------------------- (3) log-mel
def test_logmel_80_bins_max_length_vs_transformers(golden):
    g = golden("whisper_logmel80.npz")
    fe = LogMelFeatureExtractor(80, DEV)
    fe.padding = "max_length"
    f = fe(WR.waves(), sampling_rate=16000)
    feats, mask = npy(f["input_features"]), f["attention_mask"].cpu().numpy()
    assert feats.shape == (2, 80, 3000) and mask.shape == (2, 3000)
    assert np.array_equal(mask, g["attention_mask"]) and mask.sum(-1).tolist() == [1000, 301]
    d = float(np.abs(feats - g["input_features"]).max())
    print(f"log-mel 80 bins vs WhisperFeatureExtractor: max |diff| {d:.3e}")
    assert d < 5e-4
    # a clip longer than 30 s is cut to the window
    long = fe([np.concatenate([WR.waves()[0]] * 4)], sampling_rate=16000)
    assert long["input_features"].shape == (1, 80, 3000) and int(long["attention_mask"].sum()) == 3000


def test_logmel_128_bins_same_bits_with_and_without_window_padding():
    wav = OW.synthetic_wave(2, 480000)
    a = LogMelFeatureExtractor(128, DEV)
    b = LogMelFeatureExtractor(128, DEV)
    b.padding = "max_length"
    fa, fb = a([wav], sampling_rate=16000), b([wav], sampling_rate=16000)
    assert fa["input_features"].shape == (1, 128, 3000)
    assert torch.equal(fa["input_features"], fb["input_features"]) and torch.equal(fa["attention_mask"], fb["attention_mask"])


# ---------------------------------------------------------------------------- (4) true widths against transformers, live on the CPU
TINY = dict(d_model=384, encoder_attention_heads=6, encoder_ffn_dim=1536, encoder_layers=4, num_mel_bins=80, max_source_positions=1500)
LARGE_V3_2L = dict(d_model=1280, encoder_attention_heads=20, encoder_ffn_dim=5120, encoder_layers=2, num_mel_bins=128, max_source_positions=1500)


@pytest.mark.parametrize("cfg,B", [(TINY, 2), (LARGE_V3_2L, 1)], ids=["whisper-tiny", "large-v3-2-layers"])
@pytest.mark.parametrize("res_f32", [False, True], ids=["bf16-stream", "fp32-stream"])
def test_true_width_vs_transformers(cfg, B, res_f32):
    pytest.importorskip("transformers")
    sd = WR.encoder_weights(cfg, seed=5)
    x = (0.6 * np.random.RandomState(3).standard_normal((B, cfg["num_mel_bins"], 3000))).astype(np.float32)
    with torch.no_grad():
        ref = WR.hf_encoder(cfg, sd)(torch.from_numpy(x)).last_hidden_state.numpy()
    enc = WhisperEncoderMI355X(WhisperEncoderConfig(cfg), DEV).load_state_dict_hf(sd)
    enc.res_f32 = res_f32
    out = npy(enc(torch.from_numpy(x), return_f32=True).last_hidden_state)
    print(f"whisper d_model {cfg['d_model']} res_f32={res_f32}: relmax {relmax(out, ref):.5f} cosine {cosine(out, ref):.6f}")
    assert out.shape == ref.shape
    assert relmax(out, ref) < 2e-2 and cosine(out, ref) > 0.9995


# ---------------------------------------------------------------------------- (5) weights in, weights out, wrong length
def _bf16(v):
    return torch.from_numpy(np.ascontiguousarray(v)).to(torch.bfloat16).float().numpy()


@pytest.mark.parametrize("prefix", ["", "model.encoder."])
def test_state_dict_round_trip_and_length_check(prefix):
    sd = WR.encoder_weights()
    enc = WhisperEncoderMI355X(WhisperEncoderConfig(WR.SMALL), DEV).load_state_dict_hf({prefix + k: v for k, v in sd.items()})
    out = enc.export_state_dict_hf()
    assert set(out) == set(sd)
    for k, v in sd.items():
        want = _bf16(v) if (v.ndim >= 2 and k != "embed_positions.weight") else v
        assert np.array_equal(out[k], want), k
    with pytest.raises(ValueError, match="length 3000"):
        enc(torch.zeros(1, 80, 2000))


# ---------------------------------------------------------------------------- (6) the whole model around the tower
class _Tok:
    def convert_tokens_to_ids(self, t):
        return R.SMALL["audio_token_id"]


def _tiny_model(**kw):
    S = R.SMALL
    cfg = ASRConfig(audio_model_id="openai/whisper-tiny", audio_config=dict(model_type="whisper", **TINY), text_config=S["lm"],
                    projector_hidden_dim=S["proj_hidden"], audio_token_id=S["audio_token_id"], pad_token_id=S["pad_id"],
                    eos_token_id=S["eos_id"], model_dtype="float32")
    return ASRModel(cfg, device=DEV, init="random", seed=0, **kw)


def test_asr_model_with_a_whisper_tower(tmp_path):
    S = R.SMALL
    m = _tiny_model()
    assert isinstance(m.audio_tower, WhisperEncoderMI355X) and m.config.encoder_dim == 384
    fe = m.feature_extractor
    assert fe.feature_size == 80 and fe.padding == "max_length"
    f = fe(WR.waves(), sampling_rate=16000)
    feats, mask = f["input_features"], f["attention_mask"]
    assert feats.shape == (2, 80, 3000)
    # the token-count contract: mel mask -> conv formula -> projector.get_output_length
    want = m.projector.get_output_length(compute_encoder_output_length(mask.sum(-1)))
    assert want.tolist() == [125, 37]
    proc = ASRProcessor(fe, _Tok(), projector=m.projector, encoder_conv_layers=m.config.encoder_conv_layers)
    assert proc.audio_token_counts(mask).tolist() == want.tolist() and m._get_num_audio_tokens(mask) == 125
    ids, att, lab, counts = OW.synthetic_tokens(2, want.tolist(), S["lm"]["vocab"], S["audio_token_id"], S["pad_id"], S["eos_id"],
                                                n_text=20, n_suffix=8, ragged=True)
    assert counts.tolist() == want.tolist()
    batch = dict(input_ids=torch.from_numpy(ids), input_features=feats, attention_mask=torch.from_numpy(att),
                 labels=torch.from_numpy(lab), audio_token_counts=torch.from_numpy(counts))
    m.train()
    trainable = [n for n, p in m.named_parameters() if p.requires_grad]
    assert trainable and all(n.startswith("projector.") for n in trainable)
    assert not list(m.audio_tower.parameters())
    out = m(**batch, return_logits=False)
    out.loss.backward()
    grads = {n: p.grad for n, p in m.named_parameters()}
    assert all(g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for n, g in grads.items() if n.startswith("projector."))
    assert all(g is None for n, g in grads.items() if not n.startswith("projector."))
    m.zero_grad(set_to_none=True)
    tr = ASRTrainer(m, TrainingArguments(learning_rate=1e-3, weight_decay=0.0, max_grad_norm=1.0))
    losses = []
    for _ in range(3):
        tr.training_step(batch)
        losses.append(tr.last_loss())
    print("whisper-tiny ASRModel losses", losses)
    assert all(np.isfinite(losses)) and losses[2] < losses[0]
    # generation on clip 0
    prompt = np.concatenate([[5, 6, 7], [S["audio_token_id"]] * 125, [8, 9, 10, 11]]).astype(np.int64)[None]
    toks = m.generate(input_ids=torch.from_numpy(prompt), input_features=feats[:1], audio_attention_mask=mask[:1],
                      attention_mask=torch.ones(prompt.shape, dtype=torch.int64), max_new_tokens=6).cpu().numpy()
    assert toks.shape[0] == 1 and 1 <= toks.shape[1] <= 6 and (toks >= 0).all() and (toks < S["lm"]["vocab"]).all()
    # save -> load: the same tower, bit for bit
    h0 = m.audio_tower(feats).last_hidden_state
    m.save_pretrained(tmp_path)
    m2 = ASRModel.from_pretrained(tmp_path, device=DEV, init="random", seed=0)
    assert isinstance(m2.audio_tower, WhisperEncoderMI355X) and m2.feature_extractor.padding == "max_length"
    m2._apply_stream_modes()
    assert torch.equal(m2.audio_tower(feats).last_hidden_state, h0)
    for (n, a), (_, b) in zip(m.projector.named_parameters(), m2.projector.named_parameters()):
        assert torch.equal(a, b), n


def test_default_model_keeps_the_glm_tower():
    from tiny_audio_amd.encoder import GlmAsrEncoderMI355X
    S = R.SMALL
    m = ASRModel(ASRConfig(audio_config=S["enc"], text_config=S["lm"], projector_hidden_dim=S["proj_hidden"],
                           audio_token_id=S["audio_token_id"]), device=DEV, init="none")
    assert type(m.audio_tower) is GlmAsrEncoderMI355X and m.feature_extractor.padding is False


# ---------------------------------------------------------------------------- (7) the custom operator
def test_whisper_encoder_op_passes_opcheck(golden):
    x, _, _ = small_fixture(golden)
    enc = small_encoder()
    feats = torch.from_numpy(x[:1]).to(DEV)
    h = torch_ops.register_module(enc)
    torch.library.opcheck(torch.ops.ta355.whisper_encoder_forward, (feats, None, h, False), test_utils=("test_schema", "test_faketensor"))
    keep = torch.ones(1500, device=DEV)
    torch.library.opcheck(torch.ops.ta355.whisper_encoder_forward, (feats, keep, h, True), test_utils=("test_schema", "test_faketensor"))


def test_pos_add_kernel_against_torch():
    """ta_pos_add on both storage types: x[b, s, :] += pos[s, :], rounded once to the storage type."""
    import ctypes as C
    from tiny_audio_amd import _lib
    from tiny_audio_amd.ops import ptr, stream
    B, S, H = 3, 70, 128
    g = torch.Generator(device=DEV); g.manual_seed(1)
    x = torch.randn(B, S, H, device=DEV, generator=g)
    pos = torch.randn(S, H, device=DEV, generator=g)
    xf = x.clone()
    _lib.check(_lib.lib().ta_pos_add(ptr(xf), 1, ptr(pos), B, S, H, stream()))
    assert torch.equal(xf, x + pos[None])
    xb = x.to(torch.bfloat16)
    want = (xb.float() + pos[None]).to(torch.bfloat16)
    _lib.check(_lib.lib().ta_pos_add(ptr(xb), 0, ptr(pos), B, S, H, stream()))
    assert torch.equal(xb, want)
    assert _lib.lib().ta_pos_add(ptr(xb), 0, ptr(pos), B, S, 12, stream()) == 1          # H % 8

"""-m "not gpu": the Whisper audio tower's host side -- C ABI declarations and exports, the ctypes mirror of the new weights struct,
the config classes and the tower-selection rule, the packed weight images against a numpy restatement, the config JSON round trip,
and the frame-count check that must fire before any device call."""
import ctypes as C
import math
import re

import numpy as np
import pytest
import torch

from tests.golden import whisper_recipe as WR
from tiny_audio_amd import _lib
from tiny_audio_amd.asr_config import ASRConfig, EncoderConfig, WhisperEncoderConfig, is_whisper
from tiny_audio_amd.whisper_encoder import Q_SCALE, WhisperEncoderMI355X, conv1_k, pack_state_dict, sinusoids, strip_prefix

NEW_SYMBOLS = ("ta_whisper_encoder_workspace_bytes", "ta_whisper_encoder_forward", "ta_pos_add")


def test_header_declares_and_library_exports_the_new_entry_points():
    protos = _lib.parse_header()
    _lib.build()
    handle = C.CDLL(_lib.SO_PATH)
    for name in NEW_SYMBOLS:
        assert name in protos, name
        assert hasattr(handle, name), name
    # the composite takes ta_encoder_forward's argument list
    assert [C.sizeof(t) for t in protos["ta_whisper_encoder_forward"][1]] == [C.sizeof(t) for t in protos["ta_encoder_forward"][1]]
    assert len(protos["ta_whisper_encoder_workspace_bytes"][1]) == 3 and protos["ta_whisper_encoder_workspace_bytes"][0] is C.c_long
    assert _lib.lib().ta_version() == 4                       # additive: the ABI version does not move


def _header_struct(name):
    """[(c type, field)] of ``typedef struct { ... } name;`` in include/ta355.h."""
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\}\s*" + name + r"\s*;", text, flags=re.S).group(1)
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        base, rest = re.match(r"((?:const\s+)?\w+)\s*(.*)", decl, flags=re.S).groups()
        for item in rest.split(","):
            item = item.strip()
            fields.append((base + ("*" if item.startswith("*") else ""), item.lstrip("* ")))
    return fields


def test_ctypes_struct_mirrors_the_header():
    hdr = _header_struct("ta_whisper_encoder_weights")
    got = _lib.WhisperEncoderWeights._fields_
    assert [n for _, n in hdr] == [n for n, _ in got]
    for (cty, name), (_, t) in zip(hdr, got):
        want = 8 if cty.endswith("*") else 4                   # pointers, or int / float
        assert C.sizeof(t) == want, (name, cty, t)
        assert (cty == "float") == (t is C.c_float), name
    # ... and the layer struct it reuses is the GLM tower's, unchanged
    assert [n for _, n in _header_struct("ta_enc_layer")] == [n for n, _ in _lib.EncLayer._fields_]
    w = _lib.WhisperEncoderWeights(hidden=384, max_pos=1500, res_f32=1)
    assert (w.hidden, w.max_pos, w.res_f32) == (384, 1500, 1)


def test_whisper_encoder_config_sources():
    kw = WhisperEncoderConfig(d_model=768, encoder_attention_heads=12, encoder_ffn_dim=3072, encoder_layers=12)
    assert (kw.hidden_size, kw.num_attention_heads, kw.intermediate_size, kw.num_hidden_layers) == (768, 12, 3072, 12)
    assert (kw.num_mel_bins, kw.max_source_positions, kw.layer_norm_eps, kw.model_type) == (80, 1500, 1e-5, "whisper")
    d = WhisperEncoderConfig(dict(d_model=1280, encoder_attention_heads=20, encoder_ffn_dim=5120, encoder_layers=32, num_mel_bins=128))
    assert (d.hidden_size, d.num_mel_bins, d.d_model, d.encoder_layers) == (1280, 128, 1280, 32)
    transformers = pytest.importorskip("transformers")
    hf = transformers.WhisperConfig(d_model=512, encoder_attention_heads=8, encoder_ffn_dim=2048, encoder_layers=6)
    c = WhisperEncoderConfig(hf)
    assert (c.hidden_size, c.num_attention_heads, c.intermediate_size, c.num_hidden_layers, c.num_mel_bins, c.max_source_positions) == \
        (512, 8, 2048, 6, 80, 1500)
    assert isinstance(ASRConfig(audio_config=hf).audio_config, WhisperEncoderConfig)     # model_type == "whisper" on the passed config


def test_head_dim_other_than_64_is_refused():
    with pytest.raises(ValueError, match="head_dim 64"):
        WhisperEncoderConfig(d_model=384, encoder_attention_heads=4)
    with pytest.raises(ValueError, match="head_dim 64"):
        EncoderConfig(hidden_size=384, num_attention_heads=4)


def test_tower_selection_rule():
    default = ASRConfig()
    assert type(default.audio_config) is EncoderConfig and default.audio_model_id == "zai-org/GLM-ASR-Nano-2512"
    assert type(ASRConfig(audio_config=dict(hidden_size=256, num_attention_heads=4)).audio_config) is EncoderConfig
    small = ASRConfig(audio_model_id="openai/whisper-small")
    assert isinstance(small.audio_config, WhisperEncoderConfig)
    a = small.audio_config
    assert (a.hidden_size, a.num_attention_heads, a.intermediate_size, a.num_hidden_layers, a.num_mel_bins) == (768, 12, 3072, 12, 80)
    assert small.encoder_dim == 768
    v3 = ASRConfig(audio_model_id="openai/Whisper-large-v3-turbo").audio_config
    assert (v3.hidden_size, v3.num_mel_bins) == (1280, 128)
    by_type = ASRConfig(audio_config=dict(model_type="whisper", d_model=384, encoder_attention_heads=6))
    assert isinstance(by_type.audio_config, WhisperEncoderConfig)
    assert is_whisper("openai/whisper-tiny") and not is_whisper("zai-org/GLM-ASR-Nano-2512")
    assert not is_whisper("openai/whisper-tiny", EncoderConfig())                      # an explicit sub-config object wins


def test_config_json_round_trip():
    from tiny_audio_amd.checkpoint import config_from_json, config_to_json
    import json
    cfg = ASRConfig(audio_model_id="openai/whisper-tiny", audio_config=WhisperEncoderConfig(WR.SMALL),
                    text_config=dict(vocab=1024, hidden=256, ffn=512, layers=2, heads=4, kv_heads=2), projector_hidden_dim=128)
    js = json.loads(json.dumps(config_to_json(cfg)))
    assert js["audio_config"]["model_type"] == "whisper"
    back = config_from_json(js)
    assert isinstance(back.audio_config, WhisperEncoderConfig)
    assert back.audio_config.__dict__ == cfg.audio_config.__dict__ and back.text_config.__dict__ == cfg.text_config.__dict__
    assert json.loads(json.dumps(config_to_json(back))) == js                            # a second trip changes nothing
    glm = config_from_json(json.loads(json.dumps(config_to_json(ASRConfig()))))
    assert type(glm.audio_config) is EncoderConfig


def _bf16(x):
    """numpy restatement of the bf16 cast (round to nearest even) -> float32 values."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16 << 16).astype(np.uint32)
    return r.view(np.float32)


@pytest.mark.parametrize("prefix", ["", "model.encoder.", "encoder."])
def test_weight_images_equal_a_numpy_restatement(prefix):
    cfg = WhisperEncoderConfig(WR.SMALL)
    sd = WR.encoder_weights()
    given = {prefix + k: v for k, v in sd.items()}
    if prefix:
        given["model.decoder.embed_tokens.weight" if prefix.startswith("model") else "decoder.embed_tokens.weight"] = np.zeros((4, 4), np.float32)
    assert set(strip_prefix(given)) == set(sd)
    b = pack_state_dict(given, cfg)
    H, M = 128, 80
    f = lambda t: t.float().numpy()
    assert conv1_k(80) == 256 and conv1_k(128) == 384
    c1 = f(b["conv1_w"])
    assert c1.shape == (H, 256) and b["conv1_w"].dtype == torch.bfloat16
    assert np.array_equal(c1[:, 240:], np.zeros((H, 16), np.float32))
    for tap in range(3):                                        # column = tap * n_mels + cin
        assert np.array_equal(c1[:, tap * M:(tap + 1) * M], _bf16(sd["conv1.weight"][:, :, tap]))
        assert np.array_equal(f(b["conv2_w"])[:, tap * H:(tap + 1) * H], _bf16(sd["conv2.weight"][:, :, tap]))
    assert np.array_equal(f(b["pos_emb"]), sd["embed_positions.weight"]) and b["pos_emb"].dtype == torch.float32
    qs = np.float32((64 ** -0.5) * math.log2(math.e))
    assert abs(Q_SCALE - float(qs)) < 1e-7
    for i in range(2):
        a, p = f"layers.{i}.self_attn.", f"layers.{i}."
        fa = f(b[p + "wqkv_fa"])
        assert fa.shape == (3 * H, H)
        assert np.array_equal(fa[:H], _bf16(sd[a + "q_proj.weight"] * qs))              # q rows scaled, in their natural order
        assert np.array_equal(fa[H:2 * H], _bf16(sd[a + "k_proj.weight"])) and np.array_equal(fa[2 * H:], _bf16(sd[a + "v_proj.weight"]))
        bfa = f(b[p + "bqkv_fa"])
        assert np.array_equal(bfa[:H], sd[a + "q_proj.bias"] * qs) and not bfa[H:2 * H].any()
        assert np.array_equal(bfa[2 * H:], sd[a + "v_proj.bias"])
        assert np.array_equal(f(b[p + "wo"]), _bf16(sd[a + "out_proj.weight"])) and np.array_equal(f(b[p + "bo"]), sd[a + "out_proj.bias"])
        assert np.array_equal(f(b[p + "w1"]), _bf16(sd[p + "fc1.weight"])) and np.array_equal(f(b[p + "w2"]), _bf16(sd[p + "fc2.weight"]))
        assert np.array_equal(f(b[p + "ln1_w"]), sd[p + "self_attn_layer_norm.weight"])
        assert np.array_equal(f(b[p + "ln2_b"]), sd[p + "final_layer_norm.bias"])


def test_export_round_trip_on_the_cpu():
    """load_state_dict_hf -> export_state_dict_hf: exact up to the bf16 cast of the matrices (a CPU 'device': no kernel runs)."""
    cfg = WhisperEncoderConfig(WR.SMALL)
    sd = WR.encoder_weights()
    enc = WhisperEncoderMI355X(cfg, device="cpu").load_state_dict_hf({"model.encoder." + k: v for k, v in sd.items()})
    out = enc.export_state_dict_hf()
    assert set(out) == set(sd)
    for k, v in sd.items():
        want = _bf16(v) if (v.ndim >= 2 and k != "embed_positions.weight") else v
        assert np.array_equal(out[k], want), k


def test_sinusoids_match_transformers():
    mw = pytest.importorskip("transformers.models.whisper.modeling_whisper")
    assert torch.equal(sinusoids(1500, 384), mw.sinusoids(1500, 384).float())
    # the fixture recipe's float64 restatement: the float32 phase of frame 1499 carries ~1e-4 of rounding
    assert np.allclose(WR.sinusoids(1500, 128), mw.sinusoids(1500, 128).numpy(), atol=1e-3)


def test_wrong_frame_count_raises_without_a_device():
    enc = WhisperEncoderMI355X(WhisperEncoderConfig(WR.SMALL), device="cpu")     # no weights, no library call: the check comes first
    with pytest.raises(ValueError, match=r"length 3000, but found 2998"):
        enc(torch.zeros(1, 80, 2998))
    with pytest.raises(ValueError, match=r"length 3000"):
        enc._forward_impl(torch.zeros(1, 80, 200))


def test_logmel_accepts_80_bins_on_the_host_side():
    """ta_logmel_scratch_floats is a host-only query: 80 bins take the wide (64-frame) tile like 64 and 256."""
    L = _lib.lib()
    assert L.ta_logmel_scratch_floats(2, 480000, 80) == L.ta_logmel_scratch_floats(2, 480000, 64) > 0


def test_operator_is_registered_with_a_fake_kernel():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from tiny_audio_amd import torch_ops
    assert "whisper_encoder_forward" in torch_ops.OPERATORS
    s = str(torch.ops.ta355.whisper_encoder_forward.default._schema)
    assert s.startswith("ta355::whisper_encoder_forward(Tensor input_features, Tensor? frame_keep, SymInt handle, bool return_f32)")
    enc = WhisperEncoderMI355X(WhisperEncoderConfig(WR.SMALL), device="cpu")
    h = torch_ops.register_module(enc)
    with FakeTensorMode():
        y = torch.ops.ta355.whisper_encoder_forward(torch.empty(2, 80, 3000), None, h, False)
        assert y.shape == (2, 1500, 128) and y.dtype == torch.bfloat16
        assert torch.ops.ta355.whisper_encoder_forward(torch.empty(2, 80, 3000), None, h, True).dtype == torch.float32

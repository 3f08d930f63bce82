"""SmolLM3 / Llama-style text tower (no q_norm / k_norm, per-layer NoPE) without a GPU: the config surface against transformers' own
``SmolLM3Config``, the refusals, the checkpoint JSON round trip, the call sequence and struct contents under DRY_RUN, and the header's
new field.  The numerics are tests/test_gpu_smollm3.py's."""
import ctypes as C
import json
import re

import numpy as np
import pytest
import torch

from oracle import weights as OW
from tiny_audio_amd import _lib
from tiny_audio_amd.asr_config import ASRConfig, LMConfig
from tiny_audio_amd.checkpoint import config_from_json, config_to_json

ENC = OW.enc_config(hidden=256, ffn=512, layers=1, heads=4)
# 4 layers of width 512 with 4 / 1 heads: head_dim 128, layer 3 NoPE
SMOL = dict(model_type="smollm3", vocab_size=1000, hidden_size=512, intermediate_size=768, num_hidden_layers=4, num_attention_heads=4,
            num_key_value_heads=1, max_position_embeddings=256)
GEOMETRY = ("vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "num_key_value_heads", "head_dim",
            "rms_norm_eps", "rope_theta", "max_position_embeddings", "model_type", "qk_norm", "no_rope_layers")


def _geom(c):
    return {k: getattr(c, k) for k in GEOMETRY}


# ----------------------------------------------------------------------------- 1. config sources
def test_lmconfig_from_smollm3_config_dict_and_kwargs():
    from transformers import SmolLM3Config
    hf = SmolLM3Config()
    a, b = LMConfig(hf), LMConfig(hf.to_dict())
    c = LMConfig(model_type="smollm3")
    assert _geom(a) == _geom(b) == _geom(c)
    assert (a.vocab_size, a.hidden_size, a.intermediate_size, a.num_hidden_layers, a.num_attention_heads, a.num_key_value_heads) == \
           (128256, 2048, 11008, 36, 16, 4)
    assert a.head_dim == 128 and a.rms_norm_eps == 1e-6 and a.rope_theta == hf.rope_parameters["rope_theta"] == 2e6
    assert a.qk_norm is False and a.no_rope_layers == list(hf.no_rope_layers)
    assert a.nope_mask == sum(1 << i for i in range(36) if (i + 1) % 4 == 0)


@pytest.mark.parametrize("interval", [1, 2, 4])
def test_no_rope_layers_follow_transformers(interval):
    from transformers import SmolLM3Config
    hf = SmolLM3Config(num_hidden_layers=8, no_rope_layer_interval=interval)
    for src in (hf, dict(model_type="smollm3", num_hidden_layers=8, no_rope_layer_interval=interval)):
        assert LMConfig(src).no_rope_layers == list(hf.no_rope_layers), interval


def test_explicit_no_rope_layers_and_derived_head_dim():
    from transformers import SmolLM3Config
    want = [1, 0, 0, 1]
    hf = SmolLM3Config(hidden_size=512, num_attention_heads=4, num_key_value_heads=1, num_hidden_layers=4, no_rope_layers=want)
    for c in (LMConfig(hf), LMConfig(dict(SMOL, no_rope_layers=want))):
        assert c.no_rope_layers == want and c.nope_mask == 0b0110
        assert c.head_dim == 128                                          # hidden_size // num_attention_heads: SmolLM3 carries no head_dim
    with pytest.raises(ValueError, match="no_rope_layers"):
        LMConfig(dict(SMOL, no_rope_layers=[1, 0]))


def test_llama_family_has_no_norm_and_rotates_everywhere():
    from transformers import LlamaConfig
    hf = LlamaConfig(vocab_size=1000, hidden_size=512, intermediate_size=768, num_hidden_layers=3, num_attention_heads=4, num_key_value_heads=2,
                     tie_word_embeddings=True)
    for c in (LMConfig(hf), LMConfig(model_type="llama", hidden_size=512, num_attention_heads=4, num_hidden_layers=3)):
        assert c.model_type == "llama" and c.qk_norm is False and c.no_rope_layers == [1, 1, 1] and c.nope_mask == 0 and c.head_dim == 128


def test_default_lmconfig_is_todays_qwen3_object():
    c = LMConfig()
    today = dict(vocab_size=151670, hidden_size=1024, intermediate_size=3072, num_hidden_layers=28, num_attention_heads=16,
                 num_key_value_heads=8, head_dim=128, rms_norm_eps=1e-6, rope_theta=1e6, max_position_embeddings=4096)
    for k, v in today.items():
        assert getattr(c, k) == v and type(getattr(c, k)) is type(v), k
    assert c.model_type == "qwen3" and c.qk_norm is True and c.no_rope_layers == [1] * 28 and c.nope_mask == 0
    assert set(c.__dict__) == set(today) | {"model_type", "qk_norm", "no_rope_layers"}
    q = LMConfig(OW.lm_config(vocab=1000, hidden=256, ffn=512, layers=2, heads=4, kv_heads=2))      # the oracle's dict form
    assert (q.model_type, q.qk_norm, q.head_dim, q.no_rope_layers) == ("qwen3", True, 128, [1, 1])


def test_asrconfig_picks_the_family():
    a = ASRConfig(text_model_id="HuggingFaceTB/SmolLM3-3B", audio_model_id="openai/whisper-tiny")
    assert a.text_config.model_type == "smollm3" and a.text_config.hidden_size == 2048 and a.llm_dim == 2048
    assert ASRConfig().text_config.model_type == "qwen3"
    # an explicit sub-config decides by its own model_type, whatever the id says
    b = ASRConfig(text_model_id="HuggingFaceTB/SmolLM3-3B", audio_config=ENC, text_config=OW.lm_config(vocab=1000, hidden=256, ffn=512, layers=2, heads=4, kv_heads=2))
    assert b.text_config.model_type == "qwen3" and b.text_config.qk_norm
    c = ASRConfig(audio_config=ENC, text_config=SMOL)
    assert c.text_config.model_type == "smollm3" and c.text_config.no_rope_layers == [1, 1, 1, 0]


# ----------------------------------------------------------------------------- 2. refusals
@pytest.mark.parametrize("field,extra", [
    ("head_dim", dict(hidden_size=256)),                                            # 256 / 4 = 64: SmolLM2, Llama-3.2-1B
    ("attention_bias", dict(attention_bias=True)),
    ("mlp_bias", dict(mlp_bias=True)),
    ("use_sliding_window", dict(use_sliding_window=True)),
    ("rope_type", dict(rope_parameters=dict(rope_type="llama3", rope_theta=5e5, factor=32.0))),
    ("rope_type", dict(rope_scaling=dict(rope_type="yarn", factor=4.0))),
    ("tie_word_embeddings", dict(tie_word_embeddings=False)),
    ("num_hidden_layers", dict(num_hidden_layers=65)),
])
def test_refusals_name_the_field(field, extra):
    with pytest.raises(ValueError, match=field):
        LMConfig(dict(SMOL, **extra))
    with pytest.raises(ValueError, match="model_type"):
        LMConfig(model_type="gpt2")


def test_out_of_range_token_ids_raise_at_construction():
    from tiny_audio_amd.asr_modeling import ASRModel
    for name in ("audio_token_id", "pad_token_id", "eos_token_id"):
        ok = dict(audio_token_id=999, pad_token_id=990, eos_token_id=991)
        ok[name] = 151669 if name == "audio_token_id" else 1000
        with pytest.raises(ValueError, match=name):
            ASRModel(ASRConfig(audio_config=ENC, text_config=SMOL, projector_hidden_dim=128, **ok), device="cpu", init="none")
    with pytest.raises(ValueError, match="audio_token_id"):                          # the Qwen3 defaults against a SmolLM3 vocabulary
        ASRModel(ASRConfig(audio_config=ENC, text_config=SMOL, projector_hidden_dim=128), device="cpu", init="none")
    # a Qwen3 tower is constructed as before, whatever the ids
    ASRModel(ASRConfig(audio_config=ENC, text_config=OW.lm_config(vocab=1000, hidden=256, ffn=512, layers=1, heads=4, kv_heads=2),
                       projector_hidden_dim=128), device="cpu", init="none")


def test_full_finetune_of_a_no_norm_tower_is_refused():
    from tiny_audio_amd.asr_modeling import ASRModel
    with pytest.raises(NotImplementedError, match="q/k-norm"):
        ASRModel(ASRConfig(audio_config=ENC, text_config=SMOL, projector_hidden_dim=128, audio_token_id=999, pad_token_id=990,
                           eos_token_id=991, freeze_language_model=False), device="cpu", init="none")


# ----------------------------------------------------------------------------- 3. JSON round trip
def test_config_json_round_trip_and_old_json():
    cfg = ASRConfig(audio_config=ENC, text_config=dict(SMOL, no_rope_layers=[1, 0, 1, 0]), audio_token_id=999, pad_token_id=990, eos_token_id=991)
    d = json.loads(json.dumps(config_to_json(cfg)))
    assert d["text_config"]["model_type"] == "smollm3" and d["text_config"]["qk_norm"] is False
    assert d["text_config"]["no_rope_layers"] == [1, 0, 1, 0]
    back = config_from_json(d)
    assert _geom(back.text_config) == _geom(cfg.text_config)
    # a JSON written before these fields existed is a Qwen3 tower
    old = json.loads(json.dumps(config_to_json(ASRConfig(audio_config=ENC))))
    for k in ("model_type", "qk_norm", "no_rope_layers"):
        old["text_config"].pop(k)
    o = config_from_json(old).text_config
    assert _geom(o) == _geom(LMConfig())


# ----------------------------------------------------------------------------- 4. dry-run plumbing
@pytest.fixture()
def dry():
    _lib.DRY_RUN = True
    try:
        yield _lib.lib()
    finally:
        _lib.DRY_RUN = False
        _lib._LIB = None


def _model(text_config, **kw):
    from tiny_audio_amd.asr_modeling import ASRModel
    cfg = ASRConfig(audio_config=ENC, text_config=text_config, projector_hidden_dim=128, audio_token_id=999, pad_token_id=990,
                    eos_token_id=991, freeze_projector=bool(kw.get("use_lora")), **kw)
    return ASRModel(cfg, device="cpu", init="random")


def _batch():
    ids, att, lab, counts = OW.synthetic_tokens(2, [12, 12], 1000, 999, 990, 991, n_text=10, n_suffix=4)
    meta = (torch.zeros(40, dtype=torch.int32), torch.zeros(40, dtype=torch.int64), 22)
    return dict(input_ids=torch.from_numpy(ids), input_features=torch.zeros(2, 128, 100), attention_mask=torch.from_numpy(att),
                labels=torch.from_numpy(lab), audio_token_counts=torch.from_numpy(counts), label_meta=meta)


def _run(m, dry):
    dry.calls.clear()
    m.train()
    out = m(**_batch())
    out.loss.backward()
    ids = torch.tensor([[5, 6] + [999] * 12 + [7, 8]] * 2)
    m.generate(input_ids=ids, input_features=torch.zeros(2, 128, 100), audio_attention_mask=torch.ones(2, 100, dtype=torch.int64),
               attention_mask=torch.ones_like(ids), max_new_tokens=3, eos_token_id=[])
    return list(dry.calls)


QWEN_SMALL = dict(vocab_size=1000, hidden_size=512, intermediate_size=768, num_hidden_layers=4, num_attention_heads=4,
                  num_key_value_heads=1, max_position_embeddings=256)


@pytest.mark.parametrize("lora", [False, True])
def test_smollm3_issues_the_same_entry_points_as_qwen3(dry, lora):
    kw = dict(use_lora=True, lora_dropout=0.0) if lora else {}
    q = _run(_model(QWEN_SMALL, **kw), dry)
    s = _run(_model(SMOL, **kw), dry)
    assert q == s
    for name in ("ta_lm_forward_loss", "ta_lm_backward", "ta_lm_prefill", "ta_lm_decode_step"):
        assert name in s, name


def test_layers_are_bound_with_null_norms_and_the_nope_bits(dry):
    nrl = [1, 0, 1, 0]
    m = _model(dict(SMOL, no_rope_layers=nrl))
    lm = m.language_model
    assert lm._w.nope_layers == 0b1010 == sum(1 << i for i, v in enumerate(nrl) if v == 0)
    for i in range(4):
        assert lm._layers_arr[i].qn_w is None and lm._layers_arr[i].kn_w is None
        assert lm._layers_arr[i].ln_in_w and lm._layers_arr[i].wqkv
    assert not any("qn_w" in k or "kn_w" in k for k in lm._bufs)
    q = _model(QWEN_SMALL).language_model
    assert q._w.nope_layers == 0 and all(q._layers_arr[i].qn_w and q._layers_arr[i].kn_w for i in range(4))
    ll = _model(dict(SMOL, model_type="llama")).language_model
    assert ll._w.nope_layers == 0 and ll._layers_arr[0].qn_w is None


def test_state_dict_with_and_without_norm_keys(dry):
    s, q = _model(SMOL).language_model, _model(QWEN_SMALL).language_model
    sd_s, sd_q = s.export_state_dict_hf(), q.export_state_dict_hf()
    assert not any("q_norm" in k or "k_norm" in k for k in sd_s)
    assert sum("q_norm" in k for k in sd_q) == 4 and set(sd_q) - set(sd_s) == {k for k in sd_q if "_norm.weight" in k and "self_attn" in k}
    s.load_state_dict_hf(sd_s)                                                  # round trip, no norm keys needed
    np.testing.assert_array_equal(s.export_state_dict_hf()["model.layers.3.self_attn.q_proj.weight"], sd_s["model.layers.3.self_attn.q_proj.weight"])
    assert s._layers_arr[2].qn_w is None and s._w.nope_layers == 0b1000
    q.load_state_dict_hf(sd_q)
    with pytest.raises(KeyError, match=r"layers\.0\.self_attn\.q_norm\.weight"):   # stray norm keys in a SmolLM3 state dict
        s.load_state_dict_hf(sd_q)
    with pytest.raises(KeyError, match=r"layers\.0\.self_attn\.q_norm\.weight"):   # a Qwen3 one without them
        q.load_state_dict_hf(sd_s)
    with pytest.raises(NotImplementedError, match="q/k-norm"):
        s.enable_full_finetune()


# ----------------------------------------------------------------------------- 5. ABI
def test_abi_version_and_the_new_header_field():
    assert _lib.lib().ta_version() == 4
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\} ta_lm_weights;", text).group(1)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    assert decls[-1] == "unsigned long long nope_layers"                         # appended: every earlier field keeps its offset
    names = [n for n, _ in _lib.LmWeights._fields_]
    assert names[-1] == "nope_layers" and names[-2] == "dx_f32"
    assert _lib.LmWeights._fields_[-1][1] is C.c_ulonglong and _lib.LmWeights.nope_layers.offset % 8 == 0
    w = _lib.LmWeights(vocab=7)
    assert w.nope_layers == 0                                                     # a zero-initialised handle is a Qwen3 handle
    w.nope_layers = (1 << 63) | 8
    assert w.nope_layers == (1 << 63) | 8

"""The ragged encoder, host side (no GPU): the three new entry points in the header, the workspace query, the checks of
``ASRModel(ragged_encoder=True)`` and the dry-run plumbing (as tests/test_packing_host.py does for packing: arguments are marshalled
through the real ctypes prototypes, nothing is computed)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import weights as OW
from tiny_audio_amd import _lib

NEW_SYMBOLS = ("ta_attention_enc_fwd_varlen", "ta_encoder_forward_ragged", "ta_encoder_ragged_workspace_bytes")


@pytest.fixture()
def dry():
    _lib.DRY_RUN = True
    try:
        yield _lib.lib()
    finally:
        _lib.DRY_RUN = False
        _lib._LIB = None


def _model(whisper=False, **kw):
    from tiny_audio_amd.asr_config import ASRConfig, WhisperEncoderConfig
    from tiny_audio_amd.asr_modeling import ASRModel
    lm = OW.lm_config(vocab=1000, hidden=256, ffn=512, layers=2, heads=4, kv_heads=2)
    if whisper:
        enc = WhisperEncoderConfig(dict(d_model=128, encoder_ffn_dim=256, encoder_layers=1, encoder_attention_heads=2, num_mel_bins=80,
                                        max_source_positions=50))
        cfg = ASRConfig(audio_config=enc, text_config=lm, projector_hidden_dim=128, audio_token_id=999)
        return ASRModel(cfg, device="cpu", init="none", **kw)
    enc = OW.enc_config(hidden=256, ffn=512, layers=1, heads=4)
    cfg = ASRConfig(audio_config=enc, text_config=lm, projector_hidden_dim=128, audio_token_id=999)
    return ASRModel(cfg, device="cpu", init="random", **kw)


def _batch(lens=(100, 61, 37)):
    """Three clips in a T = 100 batch; every row carries 12 placeholders (the projector's rows at S = 50)."""
    A, T = 999, max(lens)
    ids = torch.tensor([[5, 6] + [A] * 12 + [7, 8, 9]] * len(lens))
    amask = (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).long()
    lab = torch.where(ids != A, ids, torch.full_like(ids, -100))
    return dict(input_ids=ids, attention_mask=torch.ones_like(ids), labels=lab, input_features=torch.zeros(len(lens), 128, T),
                audio_attention_mask=amask, audio_token_counts=torch.tensor([12] * len(lens)))


# ----------------------------------------------------------------------------- the C ABI
def test_header_declares_the_entry_points():
    protos = _lib.parse_header()
    for name in NEW_SYMBOLS:
        assert name in protos, name
    assert len(protos["ta_attention_enc_fwd_varlen"][1]) == 7
    # ta_encoder_forward's argument list with the two length tables behind (w, feats, B, T)
    old, new = protos["ta_encoder_forward"][1], protos["ta_encoder_forward_ragged"][1]
    assert len(new) == len(old) + 2 and new[:4] == old[:4] and new[6:] == old[4:]
    assert protos["ta_encoder_ragged_workspace_bytes"][0] is C.c_long
    text = open(_lib.HEADER).read()
    assert "tiny_audio/asr_modeling.py:198-200" in text          # what the ragged composite replaces: a clip encoded alone


def test_ragged_workspace_query_runs_without_a_gpu():
    L = _lib.lib()
    ew = _lib.EncoderWeights(hidden=1280, ffn=5120, n_layers=32, heads=20, n_mels=128, max_pos=1500, ln_eps=1e-5)
    # the batch of scripts/packing_bench.py: 32 clips, uniform 2-20 s, seed 0
    secs = np.random.RandomState(0).uniform(2.0, 20.0, 32)
    mel = [int(round(s * 100)) for s in secs]
    B, T = 32, max(mel)
    S = (T - 1) // 2 + 1
    rows = sum((t - 1) // 2 + 1 for t in mel)
    assert (S, rows) == (981, 19833)                                  # 0.63 of the padded B * S rows
    padded = L.ta_encoder_workspace_bytes(C.byref(ew), B, T)
    sizes = [L.ta_encoder_ragged_workspace_bytes(C.byref(ew), B, T, r) for r in (B, 1000, rows, rows + 1, B * S)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1]      # non-decreasing in rows
    assert sizes[2] < padded, (sizes[2], padded)
    assert sizes[2] >= rows * 1280 * (4 + 2 + 6 + 2) + rows * 5120 * 2                   # stream, xn, q|k|v, attention out, MLP hidden


# ----------------------------------------------------------------------------- ASRModel: the switch and its refusals
def test_switch_is_a_runtime_attribute_and_off_by_default():
    m = _model()
    assert m.ragged_encoder is False
    m.ragged_encoder = True
    assert m.ragged_encoder is True and _model(ragged_encoder=True).ragged_encoder is True
    assert "ragged_encoder" not in m.config.to_dict() if hasattr(m.config, "to_dict") else True
    assert not any("ragged" in k for k in m.state_dict())


def test_whisper_tower_refuses_the_switch_by_name():
    with pytest.raises(ValueError, match="Whisper"):
        _model(whisper=True, ragged_encoder=True)
    m = _model(whisper=True)
    with pytest.raises(ValueError, match="WhisperEncoderMI355X"):
        m.ragged_encoder = True
    assert m.ragged_encoder is False
    m.ragged_encoder = False                                          # switching it off is always allowed


def test_value_errors(dry):
    m = _model(ragged_encoder=True)
    b = _batch()
    m(**b)                                                            # the good batch passes
    with pytest.raises(ValueError, match="audio_attention_mask"):
        m(**{k: v for k, v in b.items() if k != "audio_attention_mask"})
    zero = b["audio_attention_mask"].clone(); zero[1] = 0             # a clip of length 0
    with pytest.raises(ValueError, match=r"\[1, 100\]"):
        m(**{**b, "audio_attention_mask": zero})
    wide = torch.ones(3, 101, dtype=torch.int64)                      # a mask wider than the features: a length of T + 1
    with pytest.raises(ValueError):
        m(**{**b, "audio_attention_mask": wide})
    enc = m.audio_tower
    for bad in ([100, 0, 37], [100, 101, 37], [100, 61], [100, -3, 37]):
        with pytest.raises(ValueError, match="mel_lengths"):
            enc(b["input_features"], mel_lengths=bad)
    with pytest.raises(ValueError, match="audio_attention_mask"):
        m.generate(input_ids=b["input_ids"], input_features=b["input_features"])


# ----------------------------------------------------------------------------- plumbing
def test_operator_is_registered():
    from tiny_audio_amd import torch_ops
    assert "encoder_forward_ragged" in torch_ops.OPERATORS
    s = str(torch.ops.ta355.encoder_forward_ragged.default._schema)
    assert s.startswith("ta355::encoder_forward_ragged(") and "[] mel_lengths" in s and "Tensor? frame_keep" in s
    # shapes without a GPU: the fake kernel
    from torch._subclasses.fake_tensor import FakeTensorMode
    enc = _model().audio_tower
    h = torch_ops.register_module(enc)
    with FakeTensorMode():
        y = torch.ops.ta355.encoder_forward_ragged(torch.empty(3, 128, 100), [100, 61, 37], None, h, False)
        assert y.shape == (3, 50, 256) and y.dtype == torch.bfloat16
        assert torch.ops.ta355.encoder_forward_ragged(torch.empty(3, 128, 100), [100, 61, 37], None, h, True).dtype == torch.float32


def test_the_op_receives_the_mask_row_sums(dry, monkeypatch):
    from tiny_audio_amd.trainer import ASRTrainer, TrainingArguments
    m = _model(ragged_encoder=True)
    b = _batch()
    seen = []
    real = m.audio_tower._forward_ragged_impl
    monkeypatch.setattr(m.audio_tower, "_forward_ragged_impl", lambda x, lens, *a: (seen.append(list(lens)), real(x, lens, *a))[1])
    want = b["audio_attention_mask"].sum(-1).tolist()
    assert want == [100, 61, 37]
    dry.calls.clear()
    out = m(**b)
    assert seen == [want] and out.logits.shape == (3, 17, 1000)
    assert "ta_encoder_forward_ragged" in dry.calls and "ta_encoder_forward" not in dry.calls
    m.train()
    dry.calls.clear()
    ASRTrainer(m, TrainingArguments(gradient_accumulation_steps=1)).training_step(b)
    assert seen[-1] == want and "ta_encoder_forward_ragged" in dry.calls and "ta_encoder_forward" not in dry.calls
    # generate and generate_streaming go through _prepare_generation
    kw = dict(input_ids=b["input_ids"], input_features=b["input_features"], audio_attention_mask=b["audio_attention_mask"],
              attention_mask=b["attention_mask"])
    dry.calls.clear(); seen.clear()
    m.generate(**kw, max_new_tokens=2, eos_token_id=[])
    assert seen == [want] and "ta_encoder_forward_ragged" in dry.calls and "ta_encoder_forward" not in dry.calls
    dry.calls.clear(); seen.clear()
    list(m.generate_streaming(b["input_features"][1:2], b["audio_attention_mask"][1:2], input_ids=b["input_ids"][1:2],
                              return_token_ids=True, max_new_tokens=2))
    assert seen == [[61]] and "ta_encoder_forward_ragged" in dry.calls
    # the workspace is cached per (B, T, rows)
    assert m.audio_tower._rws_key == (1, 100, 31)


def test_switch_off_calls_todays_op_with_todays_arguments(dry, monkeypatch):
    m = _model()
    b = _batch()
    seen = []
    real = m.audio_tower._forward_impl
    monkeypatch.setattr(m.audio_tower, "_forward_impl", lambda *a: (seen.append(a), real(*a))[1])
    monkeypatch.setattr(m.audio_tower, "_forward_ragged_impl", lambda *a: pytest.fail("the ragged op ran with the switch off"))
    dry.calls.clear()
    m(**b)
    assert "ta_encoder_forward" in dry.calls and "ta_encoder_forward_ragged" not in dry.calls
    (x, keep, f32), = seen
    assert x.shape == (3, 128, 100) and keep is None and f32 is False          # (input_features, frame_keep, return_f32): nothing new
    dry.calls.clear()
    m.generate(input_ids=b["input_ids"], input_features=b["input_features"], audio_attention_mask=b["audio_attention_mask"],
               attention_mask=b["attention_mask"], max_new_tokens=2, eos_token_id=[])
    assert "ta_encoder_forward" in dry.calls and "ta_encoder_forward_ragged" not in dry.calls

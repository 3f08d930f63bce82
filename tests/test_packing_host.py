"""Sequence packing, host side (no GPU): first-fit placement, the layout the collator emits, the checks of
``ASRModel.forward(segment_ids=...)`` and the dry-run plumbing of the new entry points (as tests/test_dryrun_plumbing.py does for the
existing ones: arguments are marshalled through the real ctypes prototypes, nothing is computed)."""
import numpy as np
import pytest
import torch

from oracle import weights as OW
from tiny_audio_amd import _lib
from tiny_audio_amd.collator import DataCollator, first_fit, pack_sequences


class ToyTokenizer:
    """Whitespace tokenizer with a ChatML-shaped template over a small id space (words from 10 up; <audio> and <pad> given)."""
    eos_token_id = 2

    def __init__(self, audio_id=3, pad_id=0):
        self.pad_token_id = pad_id
        self.vocab = {"<|im_start|>": 1, "<|im_end|>": 2, "<audio>": audio_id, "\n": 4}
        self._next = 10

    def _id(self, w):
        if w not in self.vocab:
            self.vocab[w] = self._next
            self._next += 1
        return self.vocab[w]

    def convert_tokens_to_ids(self, t):
        return self.vocab.get(t)

    def apply_chat_template(self, messages, tokenize=True, add_generation_prompt=False, **_):
        ids = []
        for m in messages:
            words = [w for w in m["content"].replace("<audio>", " <audio> ").split() if w]
            ids += [1, self._id(m["role"]), 4] + [self._id(w) for w in words] + [2, 4]
        if add_generation_prompt:
            ids += [1, self._id("assistant"), 4]
        return ids


class _Proj:
    def get_output_length(self, n):
        return (n - 4) // 4 + 1


def _fe(arrays, **_):
    """A feature extractor that only measures: 100 mel frames per second, padded to the longest clip."""
    T = [len(a) // 160 for a in arrays]
    feats = torch.zeros((len(arrays), 8, max(T)))
    for i, (a, t) in enumerate(zip(arrays, T)):
        feats[i, :, :t] = float(i + 1)
    att = torch.zeros((len(arrays), max(T)), dtype=torch.int64)
    for i, t in enumerate(T):
        att[i, :t] = 1
    return {"input_features": feats, "attention_mask": att}


def _clips(secs):
    return [{"audio": {"array": np.full(int(s * 16000), 0.1, np.float32)}, "text": f"clip number {i} says hello"} for i, s in enumerate(secs)]


@pytest.fixture()
def dry():
    _lib.DRY_RUN = True
    try:
        yield _lib.lib()
    finally:
        _lib.DRY_RUN = False
        _lib._LIB = None


# ----------------------------------------------------------------------------- placement and layout
def test_first_fit_in_arrival_order():
    assert first_fit([70, 58, 64, 40, 100, 192], 192) == [[0, 1, 2], [3, 4], [5]]
    assert first_fit([100, 100, 50, 92, 42], 192) == [[0, 2, 4], [1, 3]]          # 50 and 42 go back to the FIRST row with room
    assert first_fit([300, 10, 200, 182], 192) == [[0], [1, 3], [2]]              # longer than pack_to: a row of its own, never shared
    assert first_fit([], 64) == []


def test_pack_sequences_layout():
    seqs = [list(range(10, 15)), list(range(20, 23)), list(range(30, 37)), list(range(40, 42))]
    labs = [[-100, -100, 12, 13, 14], [20, 21, 22], [-100] * 4 + [34, 35, 36], [-100, 41]]
    out, order = pack_sequences(seqs, labs, pack_to=8, pad_id=99)
    assert order == [0, 1, 2, 3]
    assert out["input_ids"].tolist() == [[10, 11, 12, 13, 14, 20, 21, 22], [30, 31, 32, 33, 34, 35, 36, 99], [40, 41, 99, 99, 99, 99, 99, 99]]
    assert out["segment_ids"].tolist() == [[1] * 5 + [2] * 3, [1] * 7 + [0], [1, 1] + [0] * 6]
    assert out["position_ids"].tolist() == [[0, 1, 2, 3, 4, 0, 1, 2], [0, 1, 2, 3, 4, 5, 6, 0], [0, 1, 0, 0, 0, 0, 0, 0]]
    assert out["attention_mask"].tolist() == [[1] * 8, [1] * 7 + [0], [1, 1] + [0] * 6]
    # the label at every segment start is -100, even where the clip's own labels had one there (sequence 1 starts with 20)
    assert out["labels"].tolist() == [[-100, -100, 12, 13, 14, -100, 21, 22], [-100] * 4 + [34, 35, 36, -100], [-100, 41] + [-100] * 6]


def test_sequence_longer_than_pack_to_sets_the_row_length():
    seqs = [[1] * 5, [2] * 12, [3] * 3]
    out, order = pack_sequences(seqs, [[-100] * len(s) for s in seqs], pack_to=8, pad_id=0)
    assert order == [0, 2, 1] and tuple(out["input_ids"].shape) == (2, 12)
    assert out["segment_ids"][0].tolist() == [1] * 5 + [2] * 3 + [0] * 4 and out["segment_ids"][1].tolist() == [1] * 12


def test_collator_pack_to_none_is_todays_batch_and_packed_rows_hold_the_same_clips():
    tok = ToyTokenizer()
    feats = lambda: _clips([1.0, 2.0, 0.6, 1.5, 0.8])
    plain = DataCollator(tok, _fe, 16000, projector=_Proj())(feats())
    same = DataCollator(tok, _fe, 16000, projector=_Proj(), pack_to=None)(feats())
    assert set(plain) == set(same) == {"input_ids", "attention_mask", "labels", "prompts", "prompt_attention_mask", "input_features",
                                       "audio_attention_mask", "audio_token_counts"}
    for k in plain:
        assert torch.equal(plain[k], same[k]), k
    packed = DataCollator(tok, _fe, 16000, projector=_Proj(), pack_to=80)(feats())
    assert set(packed) == {"input_ids", "attention_mask", "labels", "segment_ids", "position_ids", "input_features", "audio_attention_mask",
                           "audio_token_counts"}
    lens = plain["attention_mask"].sum(-1).tolist()
    rows = first_fit(lens, 80)
    order = [i for r in rows for i in r]
    assert len(rows) < 5 and packed["input_ids"].shape == (len(rows), max(sum(lens[i] for i in r) for r in rows))
    assert packed["audio_token_counts"].tolist() == plain["audio_token_counts"][order].tolist()
    assert torch.equal(packed["input_features"], plain["input_features"][order])
    c = 0
    for r, row in enumerate(rows):
        for s, i in enumerate(row):
            cols = packed["segment_ids"][r] == s + 1
            keep = plain["attention_mask"][i].bool()
            assert packed["input_ids"][r][cols].tolist() == plain["input_ids"][i][keep].tolist()
            lab = plain["labels"][i][keep].clone(); lab[0] = -100
            assert packed["labels"][r][cols].tolist() == lab.tolist()
            assert packed["position_ids"][r][cols].tolist() == list(range(int(keep.sum())))
            assert int((packed["input_ids"][r][cols] == 3).sum()) == int(packed["audio_token_counts"][c])
            c += 1
    with pytest.raises(ValueError):
        DataCollator(tok, _fe, 16000, projector=_Proj(), pack_to=0)


# ----------------------------------------------------------------------------- ASRModel.forward: checks and plumbing
def _model(**over):
    from tiny_audio_amd.asr_config import ASRConfig
    from tiny_audio_amd.asr_modeling import ASRModel
    enc, lm = OW.enc_config(hidden=256, ffn=512, layers=1, heads=4), OW.lm_config(vocab=1000, hidden=256, ffn=512, layers=2, heads=4, kv_heads=2)
    cfg = ASRConfig(audio_config=enc, text_config=lm, projector_hidden_dim=128, audio_token_id=999, **over)
    return ASRModel(cfg, device="cpu", init="random")


def _packed_inputs():
    """Two rows, three clips: [12 + 9 placeholders] and [12], 100 mel frames per clip (12 projector rows)."""
    A = 999
    seg = [[5, 6] + [A] * 12 + [7, 8, 9], [5] + [A] * 9 + [7, 8], [5, 6] + [A] * 12 + [7, 8, 9, 10]]
    L = len(seg[0]) + len(seg[1])
    ids = torch.zeros((2, L), dtype=torch.int64); sid = torch.zeros((2, L), dtype=torch.int64)
    ids[0, :17] = torch.tensor(seg[0]); ids[0, 17:29] = torch.tensor(seg[1]); sid[0, :17] = 1; sid[0, 17:29] = 2
    ids[1, :18] = torch.tensor(seg[2]); sid[1, :18] = 1
    lab = torch.where((ids != A) & (sid != 0), ids, torch.full_like(ids, -100))
    return dict(input_ids=ids, segment_ids=sid, attention_mask=(sid != 0).long(), labels=lab, input_features=torch.zeros(3, 128, 100),
                audio_token_counts=torch.tensor([12, 9, 12]))


def test_forward_rejects_bad_packed_batches(dry):
    m = _model()
    b = _packed_inputs()
    m(**b)                                                            # the good batch passes
    bad = lambda **kw: {**b, **kw}
    s = b["segment_ids"]
    gap = s.clone(); gap[0, 17:29] = 3                                # 1, 3: a gap
    down = s.clone(); down[0, :17] = 2; down[0, 17:29] = 1            # decreasing
    hole = s.clone(); hole[0, 5] = 0                                  # padding inside a clip
    start = s.clone(); start[1, :18] = 2                              # a row that does not start at 1
    for wrong in (gap, down, hole, start, s[:, :-1], s.float()):
        with pytest.raises(ValueError, match="segment_ids"):
            m(**bad(segment_ids=wrong, attention_mask=None))
    att = b["attention_mask"].clone(); att[1, 20] = 1
    with pytest.raises(ValueError, match="attention_mask disagrees"):
        m(**bad(attention_mask=att))
    with pytest.raises(ValueError, match="placeholders"):
        m(**bad(audio_token_counts=torch.tensor([12, 8, 12])))
    with pytest.raises(ValueError, match="placeholders"):
        m(**bad(input_features=torch.zeros(2, 128, 100), audio_token_counts=torch.tensor([12, 9])))
    with pytest.raises(ValueError, match="label_meta"):
        m(**b, label_meta=(torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int64), 2))


@pytest.mark.parametrize("mode", ["frozen", "lora", "lora_dropout", "full"])
def test_packed_training_step_plumbing(dry, mode):
    from tiny_audio_amd.trainer import ASRTrainer, TrainingArguments
    over = {"frozen": {}, "lora": dict(use_lora=True), "lora_dropout": dict(use_lora=True, lora_dropout=0.1),
            "full": dict(freeze_language_model=False)}[mode]
    m = _model(**over)
    b = _packed_inputs()
    m.train()
    dry.calls.clear()
    out = m(**b)
    assert out.logits.shape == (2, b["input_ids"].shape[1], 1000)
    out.loss.backward()
    for must in ("ta_segment_table", "ta_audio_index_seg", "ta_lm_forward_loss_seg", "ta_lm_backward_seg"):
        assert must in dry.calls, must
    assert not {"ta_audio_index", "ta_lm_forward_loss", "ta_lm_forward_loss_ex", "ta_lm_backward", "ta_lm_backward_ex"} & set(dry.calls)
    # the trainer hands the new keys to the model as they are
    dry.calls.clear()
    ASRTrainer(m, TrainingArguments(gradient_accumulation_steps=1)).training_step(b)
    assert "ta_lm_forward_loss_seg" in dry.calls and "ta_lm_backward_seg" in dry.calls
    # ... and without segment_ids the existing entry points are the ones that run
    dry.calls.clear()
    plain = {k: v for k, v in b.items() if k != "segment_ids"}
    plain["input_features"], plain["audio_token_counts"] = torch.zeros(2, 128, 100), torch.tensor([21, 12])
    m(**plain, label_meta=(torch.zeros(8, dtype=torch.int32), torch.zeros(8, dtype=torch.int64), 4)).loss.backward()
    assert not any(c.endswith("_seg") or c == "ta_segment_table" for c in dry.calls)
    assert "ta_audio_index" in dry.calls


def test_new_operators_are_registered():
    from tiny_audio_amd import torch_ops
    assert {"lm_forward_loss", "lm_backward"} <= set(torch_ops.OPERATORS)
    s = str(torch.ops.ta355.lm_forward_loss.default._schema)
    assert "Tensor? seg" in s and "Tensor? pos" in s and "float lora_p" in s
    assert "Tensor? seg" in str(torch.ops.ta355.lm_backward.default._schema)
    # one pair serves packed rows and LoRA dropout: the per-option copies are gone
    for gone in (op + option for op in ("lm_forward_loss", "lm_backward") for option in ("_drop", "_seg")):
        assert not hasattr(torch_ops, gone) and gone not in torch_ops.OPERATORS, gone

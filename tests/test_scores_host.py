"""Decoding scores, host side (no GPU): the dry-run plumbing of ``ta_token_scores_f32`` in the decode loop (arguments are marshalled
through the real ctypes prototypes, nothing is computed: tests/test_dryrun_plumbing.py), the output object of
``ASRModel.generate(return_token_scores=True)``, the streaming pairs, the operator's registration and argument checks, and the word
confidence of ``tiny_audio_amd/confidence.py``."""
import math

import pytest
import torch

from oracle import weights as OW
from tiny_audio_amd import _lib


@pytest.fixture()
def dry():
    _lib.DRY_RUN = True
    try:
        yield _lib.lib()
    finally:
        _lib.DRY_RUN = False
        _lib._LIB = None


def _model():
    from tiny_audio_amd.asr_config import ASRConfig
    from tiny_audio_amd.asr_modeling import ASRModel
    enc, lm = OW.enc_config(hidden=256, ffn=512, layers=1, heads=4), OW.lm_config(vocab=1000, hidden=256, ffn=512, layers=2, heads=4, kv_heads=2)
    cfg = ASRConfig(audio_config=enc, text_config=lm, projector_hidden_dim=128, audio_token_id=999, pad_token_id=990, eos_token_id=991)
    m = ASRModel(cfg, device="cpu", init="random")
    ids = torch.tensor([[5, 6] + [999] * 12 + [7, 8]] * 2)
    kw = dict(input_ids=ids, input_features=torch.zeros(2, 128, 100), audio_attention_mask=torch.ones(2, 100, dtype=torch.int64),
              attention_mask=torch.ones_like(ids))
    return m, kw


def test_scores_kernel_is_launched_once_per_step_before_the_bookkeeping(dry):
    m, kw = _model()
    dry.calls.clear()
    out = m.generate(**kw, max_new_tokens=5, eos_token_id=[], return_token_scores=True)
    calls = [c for c in dry.calls if c in ("ta_argmax_f32", "ta_token_scores_f32", "ta_greedy_advance")]
    assert calls == ["ta_argmax_f32", "ta_token_scores_f32", "ta_greedy_advance"] * 5      # selection, scores, then the step counter moves
    assert dry.calls.count("ta_lm_prefill") == 1 and dry.calls.count("ta_lm_decode_step") == 4
    assert not torch.is_tensor(out)
    # sampling: the scores follow the draw
    dry.calls.clear()
    m.generate(**kw, max_new_tokens=3, eos_token_id=[], do_sample=True, top_k=5, seed=1, top_logprobs=2)
    calls = [c for c in dry.calls if c in ("ta_logits_warp", "ta_sample_f32", "ta_token_scores_f32", "ta_greedy_advance")]
    assert calls == ["ta_logits_warp", "ta_sample_f32", "ta_token_scores_f32", "ta_greedy_advance"] * 3


def test_switches_off_launch_nothing_new_and_return_a_tensor(dry):
    m, kw = _model()
    dry.calls.clear()
    out = m.generate(**kw, max_new_tokens=5, eos_token_id=[])
    assert dry.calls.count("ta_token_scores_f32") == 0 and dry.calls.count("ta_greedy_advance") == 5
    assert torch.is_tensor(out) and out.shape == (2, 5) and out.dtype == torch.int64
    out = m.generate(**kw, max_new_tokens=5, eos_token_id=[], return_token_scores=False, top_logprobs=0)
    assert torch.is_tensor(out) and dry.calls.count("ta_token_scores_f32") == 0


def test_generation_output_shapes_and_dtypes(dry):
    from tiny_audio_amd.asr_modeling import GenerationOutput
    m, kw = _model()
    o = m.generate(**kw, max_new_tokens=5, eos_token_id=[], return_token_scores=True)
    assert isinstance(o, GenerationOutput) and isinstance(o, dict)
    assert list(o) == ["sequences", "token_logprobs", "token_entropy"] and o.top_token_ids is None and o.top_logprobs is None
    assert o.sequences.shape == (2, 5) and o.sequences.dtype == torch.int64
    assert o.token_logprobs.shape == (2, 5) and o.token_logprobs.dtype == torch.float32
    assert o.token_entropy.shape == (2, 5) and o.token_entropy.dtype == torch.float32
    assert o["sequences"] is o.sequences is o[0] and "scores" not in o
    with pytest.raises(AttributeError):
        o.scores                                         # HF's name for the full [B, V] rows: deliberately absent
    o = m.generate(**kw, max_new_tokens=5, eos_token_id=[], top_logprobs=3)          # alternatives alone switch the scores on too
    assert list(o) == ["sequences", "token_logprobs", "token_entropy", "top_token_ids", "top_logprobs"]
    assert o.top_token_ids.shape == (2, 5, 3) and o.top_token_ids.dtype == torch.int64
    assert o.top_logprobs.shape == (2, 5, 3) and o.top_logprobs.dtype == torch.float32
    # pad is an eos id by default: the run stops after step 0 and EVERY buffer is trimmed to the same n_new
    o = m.generate(**kw, max_new_tokens=5, return_token_scores=True, top_logprobs=8)
    assert o.sequences.shape == (2, 1) and o.token_logprobs.shape == (2, 1) and o.token_entropy.shape == (2, 1)
    assert o.top_token_ids.shape == (2, 1, 8) and o.top_logprobs.shape == (2, 1, 8)
    o = m.generate(**kw, max_new_tokens=0, return_token_scores=True, top_logprobs=2)
    assert o.sequences.shape == (2, 0) and o.token_logprobs.shape == (2, 0) and o.top_token_ids.shape == (2, 0, 2)
    # the loop's own interface
    args = m._prepare_generation(kw["input_ids"], kw["input_features"], kw["audio_attention_mask"], kw["attention_mask"], None,
                                 dict(max_new_tokens=4, eos_token_id=[]))
    seq, sc = m.language_model.greedy_decode(**args, token_scores=True, top_logprobs=4, use_graph=False)
    assert seq.shape == (2, 4) and set(sc) == {"token_logprobs", "token_entropy", "top_token_ids", "top_logprobs"}
    assert sc["top_logprobs"].shape == (2, 4, 4)
    assert torch.is_tensor(m.language_model.greedy_decode(**args))


def test_top_logprobs_out_of_range_is_refused(dry):
    m, kw = _model()
    for bad in (9, -1):
        with pytest.raises(ValueError, match="top_logprobs"):
            m.generate(**kw, max_new_tokens=5, top_logprobs=bad)
    args = m._prepare_generation(kw["input_ids"], kw["input_features"], kw["audio_attention_mask"], kw["attention_mask"], None,
                                 dict(max_new_tokens=4))
    with pytest.raises(ValueError, match="top_logprobs"):
        m.language_model.greedy_decode(**args, top_logprobs=9)
    assert m.generate(**kw, max_new_tokens=2, eos_token_id=[], top_logprobs=8).top_logprobs.shape == (2, 2, 8)


def test_streaming_yields_id_logprob_pairs(dry):
    m, kw = _model()
    one = dict(input_ids=kw["input_ids"][:1], input_features=torch.zeros(1, 128, 100), audio_attention_mask=torch.ones(1, 100, dtype=torch.int64))
    dry.calls.clear()
    got = list(m.generate_streaming(**one, return_token_ids=True, return_token_scores=True, max_new_tokens=5, eos_token_id=[]))
    assert len(got) == 5 and all(isinstance(p, tuple) and len(p) == 2 for p in got)
    assert [p[0] for p in got] == [990] * 5 and all(isinstance(p[0], int) and isinstance(p[1], float) for p in got)
    assert dry.calls.count("ta_token_scores_f32") == 5 and dry.calls.count("ta_lm_decode_step") == 4
    assert len(list(m.generate_streaming(**one, return_token_ids=True, return_token_scores=True, max_new_tokens=5))) == 1   # pad is an eos id
    dry.calls.clear()
    assert list(m.generate_streaming(**one, return_token_ids=True, max_new_tokens=5, eos_token_id=[])) == [990] * 5          # unchanged
    assert dry.calls.count("ta_token_scores_f32") == 0
    with pytest.raises(ValueError, match="return_token_ids"):
        next(m.generate_streaming(**one, return_token_scores=True))


def test_operator_is_registered_and_checks_its_arguments(dry):
    from torch._subclasses.fake_tensor import FakeTensorMode
    from tiny_audio_amd import ops, torch_ops
    assert "token_scores" in torch_ops.OPERATORS
    s = str(torch.ops.ta355.token_scores.default._schema)
    assert s.startswith("ta355::token_scores(Tensor logits, Tensor chosen, SymInt V, SymInt top_k) -> (Tensor, Tensor, Tensor, Tensor)"), s
    with FakeTensorMode():
        lp, ent, ids, tl = torch.ops.ta355.token_scores(torch.empty(3, 128), torch.empty(3, dtype=torch.int64), 100, 4)
        assert lp.shape == ent.shape == (3,) and lp.dtype == torch.float32
        assert ids.shape == (3, 4) and ids.dtype == torch.int64 and tl.shape == (3, 4) and tl.dtype == torch.float32
    x, c = torch.zeros(3, 128), torch.tensor([0, 5, 99])
    dry.calls.clear()
    lp, ent, ids, tl = ops.token_scores(x, c, 100, 2)
    assert dry.calls == ["ta_token_scores_f32"] and lp.shape == (3,) and ids.shape == (3, 2)
    lp, ent, ids, tl = ops.token_scores(x[:, :120], c, 100, 0)                 # strided rows are fine, no alternatives
    assert ids.shape == (3, 0) and tl.shape == (3, 0)
    for bad in (lambda: ops.token_scores(x.double(), c, 100, 2), lambda: ops.token_scores(x[0], c, 100, 2),
                lambda: ops.token_scores(x.t(), c, 3, 2), lambda: ops.token_scores(x, c, 129, 2), lambda: ops.token_scores(x, c, 0, 2),
                lambda: ops.token_scores(x, c.int(), 100, 2), lambda: ops.token_scores(x, c[:2], 100, 2),
                lambda: ops.token_scores(x, torch.tensor([0, 5, 100]), 100, 2), lambda: ops.token_scores(x, torch.tensor([0, -1, 3]), 100, 2),
                lambda: ops.token_scores(x, c, 100, 9), lambda: ops.token_scores(x, c, 100, -1)):
        with pytest.raises(ValueError):
            bad()
    # the header's contract
    import re
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    assert "int ta_token_scores_f32(const float* logits, long ld, int V, int B, const long* chosen, const int* finished, const int* step_dev," in text
    assert len(_lib.parse_header()["ta_token_scores_f32"][1]) == 14


# ----------------------------------------------------------------------------- word confidence
_VOCAB = {1: "hel", 2: "lo", 3: " wor", 4: "ld", 5: " ", 6: "a b", 7: "c", 20: b"\xe4\xbd", 21: b"\xa0", 22: " ok", 30: "<eos>", 31: "<pad>"}


def _decode(ids):
    """A byte-level stub: pieces are joined as bytes, an unfinished multi-byte character decodes to U+FFFD."""
    raw = b"".join(p if isinstance(p, bytes) else p.encode() for p in (_VOCAB[i] for i in ids))
    return raw.decode("utf-8", errors="replace")


def test_word_confidences_groups_tokens_into_words():
    from tiny_audio_amd.confidence import word_confidences
    lg = math.log
    # a multi-token word, a whitespace-only token, eos and pad ignored
    ids = [1, 2, 5, 3, 4, 30, 31, 31]
    lps = [lg(0.5), lg(0.25), lg(0.01), lg(0.8), lg(0.2), lg(0.9), 0.0, 0.0]
    w = word_confidences(torch.tensor(ids), torch.tensor(lps, dtype=torch.float64), [30, 31], _decode)
    assert [e["word"] for e in w] == _decode(ids[:5]).split() == ["hello", "world"]
    assert [e["n_tokens"] for e in w] == [2, 2]                         # the lone space (p = 0.01) belongs to no word
    assert w[0]["logprob"] == pytest.approx(lg(0.5) + lg(0.25)) and w[0]["confidence"] == pytest.approx(math.sqrt(0.125))
    assert w[0]["min_prob"] == pytest.approx(0.25)
    assert w[1]["logprob"] == pytest.approx(lg(0.8) + lg(0.2)) and w[1]["confidence"] == pytest.approx(0.4) and w[1]["min_prob"] == pytest.approx(0.2)
    assert set(w[0]) == {"word", "logprob", "confidence", "min_prob", "n_tokens"}
    # a token spanning two words counts in both
    w = word_confidences([1, 6, 7], [lg(0.5), lg(0.1), lg(0.4)], [30], _decode)
    assert [e["word"] for e in w] == ["hela", "bc"] and [e["n_tokens"] for e in w] == [2, 2]
    assert w[0]["logprob"] == pytest.approx(lg(0.5) + lg(0.1)) and w[1]["logprob"] == pytest.approx(lg(0.1) + lg(0.4))
    assert w[0]["min_prob"] == pytest.approx(0.1) and w[1]["min_prob"] == pytest.approx(0.1)
    # a multi-byte character split over two tokens: the held-back prefix's token shares the character
    assert _decode([20]) == "\ufffd" and _decode([20, 21]) == "\u4f60"
    w = word_confidences([20, 21, 22], [lg(0.5), lg(0.5), lg(0.9)], [30], _decode)
    assert [e["word"] for e in w] == ["\u4f60", "ok"] and [e["n_tokens"] for e in w] == [2, 1]
    assert w[0]["confidence"] == pytest.approx(0.5) and w[1]["confidence"] == pytest.approx(0.9)
    # nothing but eos / pad; a -inf token (a banned id somebody forced) gives confidence 0, not an error
    assert word_confidences([30, 31], [0.0, 0.0], [30, 31], _decode) == []
    w = word_confidences([1, 2], [float("-inf"), lg(0.5)], [], _decode)
    assert w[0]["confidence"] == 0.0 and w[0]["min_prob"] == 0.0 and w[0]["logprob"] == float("-inf")
    with pytest.raises(ValueError):
        word_confidences([1, 2], [0.0], [], _decode)


def test_attach_confidence_and_its_mismatch_error():
    from tiny_audio_amd.confidence import attach_confidence, word_confidences
    conf = word_confidences([1, 2, 3, 4], [math.log(0.5)] * 4, [30], _decode)
    words = [{"word": "hello", "start": 0.0, "end": 0.4}, {"word": "world", "start": 0.5, "end": 0.9}]
    out = attach_confidence(words, conf)
    assert out is words and [w["confidence"] for w in words] == [pytest.approx(0.5)] * 2 and words[0]["start"] == 0.0
    with pytest.raises(ValueError, match="word 1 .*'word'.*'world'"):
        attach_confidence([{"word": "hello"}, {"word": "word"}], conf)
    with pytest.raises(ValueError, match="word 1 .*'world'"):                   # the aligned text was shortened
        attach_confidence([{"word": "hello"}], conf)

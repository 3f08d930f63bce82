"""Beam search plumbing without a GPU (dry-run marshalling, as tests/test_decode_options_host.py): the launch sequence of a
``generate_beams`` step, the refusals, ``generate`` unchanged, the config fallbacks and ``GenerationOutput`` with ``sequences_scores``."""
import copy
import pickle

import pytest
import torch

from tiny_audio_amd import _lib, ops
from tests.test_decode_options_host import STEP, _model, _step_calls, dry  # noqa: F401

BEAM = ("ta_beam_logprobs_f32", "ta_beam_topk_f32", "ta_beam_advance", "ta_kv_beam_reorder")
ALL = STEP + BEAM + ("ta_lm_prefill", "ta_kv_beam_expand", "ta_lm_decode_step")


def _calls(dry):  # noqa: F811
    return [c for c in dry.calls if c in ALL]


def test_launch_sequence_of_a_beam_run(dry):  # noqa: F811
    m, kw = _model()
    dry.calls.clear()
    out = m.generate_beams(**kw, max_new_tokens=3, eos_token_id=[991], num_beams=4, num_return_sequences=2)
    select = list(BEAM)
    assert _calls(dry) == ["ta_lm_prefill", "ta_kv_beam_expand"] + select + (["ta_lm_decode_step"] + select) * 2
    assert out.sequences.shape[0] == 4 and out.sequences.dtype == torch.int64 and out.sequences_scores.shape == (4,)
    assert "ta_argmax_f32" not in dry.calls and "ta_greedy_advance" not in dry.calls
    # the processors sit between the log-softmax and the top-k, in HF's order, on the rows of the beams
    dry.calls.clear()
    m.generate_beams(**kw, max_new_tokens=2, eos_token_id=[991], num_beams=2, sequence_bias={(5,): 2.0}, repetition_penalty=1.2,
                     bad_words_ids=[[6, 7]], min_new_tokens=1, suppress_tokens=[1])
    step = ["ta_beam_logprobs_f32", "ta_logits_sequence_bias", "ta_logits_process", "ta_logits_sequence_bias", "ta_logits_suppress_until",
            "ta_logits_step_rules", "ta_beam_topk_f32", "ta_beam_advance", "ta_kv_beam_reorder"]
    assert _calls(dry) == ["ta_lm_prefill", "ta_kv_beam_expand"] + step + ["ta_lm_decode_step"] + step
    # one beam moves no cache rows
    dry.calls.clear()
    m.generate_beams(**kw, max_new_tokens=2, eos_token_id=[], num_beams=1)
    assert dry.calls.count("ta_kv_beam_reorder") == 0 and dry.calls.count("ta_beam_advance") == 2
    # the trace comes back as a second item
    out, tr = m.generate_beams(**kw, max_new_tokens=2, eos_token_id=[], num_beams=2, return_beam_trace=True)
    assert tr["n_steps"] == 2 and tr["cand_score"].shape == (2, 2, 4) and tr["running_sequences"].shape == (2, 2, 2, 2)


def test_generate_is_unchanged_and_keeps_raising(dry):  # noqa: F811
    m, kw = _model()
    dry.calls.clear()
    m.generate(**kw, max_new_tokens=4, eos_token_id=[], num_beams=1, length_penalty=2.0)
    assert _step_calls(dry) == ["ta_argmax_f32", "ta_greedy_advance"] * 4 and not any(c in BEAM or c == "ta_kv_beam_expand" for c in dry.calls)
    with pytest.raises(NotImplementedError, match="generate_beams"):
        m.generate(**kw, max_new_tokens=4, num_beams=2)
    m.config.num_beams = 3
    with pytest.raises(NotImplementedError, match="generate_beams"):
        m.generate(**kw, max_new_tokens=4)
    one = dict(input_features=kw["input_features"][:1], audio_attention_mask=kw["audio_attention_mask"][:1], input_ids=kw["input_ids"][:1])
    with pytest.raises(ValueError, match="num_beams"):
        list(m.generate_streaming(**one, return_token_ids=True, max_new_tokens=2))
    with pytest.raises(ValueError, match="num_beams"):
        list(m.generate_streaming(**one, return_token_ids=True, max_new_tokens=2, num_beams=2))


def test_refusals(dry):  # noqa: F811
    m, kw = _model()
    g = lambda **o: m.generate_beams(**kw, max_new_tokens=3, eos_token_id=[991], **o)  # noqa: E731
    for o, match in ((dict(num_beams=2, do_sample=True), "beam sampling"), (dict(num_beams=2, return_token_scores=True), "sequences_scores"),
                     (dict(num_beams=2, top_logprobs=3), "sequences_scores"), (dict(num_beams=2, num_return_sequences=3), "num_return_sequences"),
                     (dict(num_beams=4, num_beam_groups=2), "num_beam_groups"), (dict(num_beams=2, constraints=[object()]), "constraints"),
                     (dict(num_beams=2, force_words_ids=[[5]]), "force_words_ids"), (dict(num_beams=9), r"within \[1, 8\]"),
                     (dict(num_beams=0), r"within \[1, 8\]"), (dict(num_beams=2, early_stopping="sometimes"), "early_stopping"),
                     (dict(num_beams=2, bad_words_ids=[[1000]]), "vocabulary size is 1000")):
        dry.calls.clear()
        with pytest.raises(ValueError, match=match):
            g(**o)
        assert not any(c in ALL for c in dry.calls), o
    with pytest.raises(ValueError, match="at most 3 eos"):
        m.generate_beams(**kw, max_new_tokens=3, eos_token_id=[1, 2, 3, 4], num_beams=2)


def test_config_fallbacks(dry):  # noqa: F811
    m, kw = _model()
    m.config.num_beams, m.config.length_penalty, m.config.early_stopping = 2, 2.0, "never"
    seen = {}
    real = m.language_model.beam_decode
    m.language_model.beam_decode = lambda **a: (seen.update(a), real(**a))[1]
    m.generate_beams(**kw, max_new_tokens=2, eos_token_id=[991])
    assert (seen["num_beams"], seen["length_penalty"], seen["early_stopping"]) == (2, 2.0, "never")
    m.generate_beams(**kw, max_new_tokens=2, eos_token_id=[991], num_beams=3, length_penalty=0.0, early_stopping=True)       # the call first
    assert (seen["num_beams"], seen["length_penalty"], seen["early_stopping"]) == (3, 0.0, True)
    m.config.num_beams, m.config.length_penalty, m.config.early_stopping = None, None, None
    m.generate_beams(**kw, max_new_tokens=2, eos_token_id=[991])
    assert (seen["num_beams"], seen["length_penalty"], seen["early_stopping"]) == (1, 1.0, False)


def test_generation_output_round_trip():
    from tiny_audio_amd.asr_modeling import GenerationOutput
    seq, sc = torch.arange(6).reshape(2, 3), torch.tensor([-1.5, -2.5])
    o = GenerationOutput(sequences=seq, sequences_scores=sc)
    assert list(o) == ["sequences", "sequences_scores"] and o.sequences_scores is sc and o[1] is sc and o.token_logprobs is None
    assert GenerationOutput._items[-1] == "sequences_scores" and GenerationOutput._items[:5] == ("sequences", "token_logprobs", "token_entropy",
                                                                                                  "top_token_ids", "top_logprobs")
    for c in (copy.deepcopy(o), pickle.loads(pickle.dumps(o)), GenerationOutput(dict(o))):
        assert isinstance(c, GenerationOutput) and list(c) == list(o) and torch.equal(c.sequences_scores, sc) and torch.equal(c["sequences"], seq)
    assert GenerationOutput(seq, None, None, None, None).sequences_scores is None      # the five positional items of before still bind


def test_wrappers_operators_and_header(dry):  # noqa: F811
    from tiny_audio_amd import torch_ops
    assert {"beam_logprobs", "beam_topk", "beam_advance", "kv_beam_expand", "kv_beam_reorder"} <= set(torch_ops.OPERATORS)
    assert "Tensor(a0!) logits" in str(torch.ops.ta355.beam_logprobs.default._schema)
    x = torch.zeros(8, 128)
    dry.calls.clear()
    assert ops.beam_logprobs(x, 100) is x
    cs, cf = ops.beam_topk(x, 100, torch.zeros(2, 4), 8)
    assert cs.shape == (2, 8) and cf.dtype == torch.int32
    kd, vd = ops.kv_beam_expand(torch.zeros(1, 2, 1, 3, 128, dtype=torch.bfloat16), torch.zeros(1, 2, 1, 3, 128, dtype=torch.bfloat16), 4, 7)
    assert kd.shape == (1, 8, 1, 7, 128)
    ops.kv_beam_reorder(kd, vd, 4, 3, 4, torch.zeros(8, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))
    torch.ops.ta355.beam_topk(x, 100, torch.zeros(2, 4), 8)
    assert dry.calls == ["ta_beam_logprobs_f32", "ta_beam_topk_f32", "ta_kv_beam_expand", "ta_kv_beam_reorder", "ta_beam_topk_f32"]
    for bad in (lambda: ops.beam_topk(x, 100, torch.zeros(2, 4), 33), lambda: ops.beam_topk(x, 100, torch.zeros(3, 3), 6),
                lambda: ops.beam_logprobs(x.double(), 100), lambda: ops.kv_beam_expand(kd.float(), vd.float(), 2, 9),
                lambda: ops.kv_beam_reorder(kd, vd, 4, 3, 5, torch.zeros(8, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)),
                lambda: ops.beam_candidates(9, 1), lambda: ops.beam_candidates(2, 4)):
        with pytest.raises(ValueError):
            bad()
    assert ops.beam_candidates(4, 0) == 8 and ops.beam_candidates(4, 3) == 16
    assert ops.beam_length_divisors(2.0, 3).tolist() == [1.0, 4.0, 9.0] and ops.beam_length_divisors(0.0, 2).tolist() == [1.0, 1.0]
    protos = _lib.parse_header()
    assert len(protos["ta_beam_advance"][1]) == 35 and len(protos["ta_beam_topk_f32"][1]) == 12 and len(protos["ta_kv_beam_reorder"][1]) == 13
    assert _lib.lib().ta_version() == 4
    text = open(_lib.HEADER).read()
    for fn in ("_get_top_k_continuations", "_get_running_beams_for_next_iteration", "_update_finished_beams", "_check_early_stop_heuristic",
               "_beam_search_has_unfinished_sequences"):
        assert fn in text, fn

"""Decoding options, host side (no GPU): the numpy restatement of tests/decode_options_ref.py against HF's own outputs
(tests/golden/decode_options.npz: bit-identical for the bias, bad-word and step rules and for HF's whole processor list; the float64
warpers against HF's float32 ones within the recorded bands), the sequence-table builder, every ValueError, the dry-run launch
sequence of ``ASRModel.generate`` with each option (HF's order) and with none (unchanged), and the operators' registration."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import weights as OW
from tests import decode_options_ref as R
from tiny_audio_amd import _lib, ops

C = R.CASES
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_options.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def same(a, b):
    """bit-identical up to the sign of zero (HF's ``scores + 0`` turns -0.0 into +0.0), NaN == NaN"""
    return np.array_equal(np.asarray(a, np.float32), np.asarray(b, np.float32), equal_nan=True)


# ----------------------------------------------------------------------------- the restatement against HF
def test_fixture_inputs_are_the_shared_cases(gold):
    assert np.array_equal(gold["scores"], C.scores(), equal_nan=True) and np.array_equal(gold["context"], C.context())
    assert os.path.getsize(GOLD) < 1 << 20


def test_bias_bad_words_and_step_rules_are_bit_identical_to_hf(gold):
    x, ctx = gold["scores"], gold["context"]
    assert same(R.sequence_bias(x, ctx, C.SEQUENCE_BIAS), gold["sequence_bias"])
    assert same(R.sequence_bias(x, ctx[:, C.L:], C.SEQUENCE_BIAS), gold["sequence_bias_generated_only"])
    assert same(R.sequence_bias(x, ctx, C.SEQUENCE_BIAS_LIST_FORM), gold["sequence_bias_list_form"])
    assert not same(gold["sequence_bias"], gold["sequence_bias_generated_only"])             # the straddling entry fired with the prompt only
    assert gold["sequence_bias"][0, 60] == x[0, 60] + np.float32(1.0)                         # (1e8 - 1e8) + 1: the order is visible
    assert gold["sequence_bias"][0, 71] == x[0, 71] + np.float32(5.0) and gold["sequence_bias_generated_only"][0, 71] == x[0, 71]
    assert gold["sequence_bias"][0, 72] == x[0, 72]                                           # longer than the context: skipped
    assert np.isneginf(gold["sequence_bias"][:, 80]).all() and np.isneginf(gold["sequence_bias"][0, 90])
    assert same(R.bad_words(x, ctx, C.BAD_WORDS, C.EOS), gold["bad_words"])
    assert np.isfinite(gold["bad_words"][:, 7]).all() and np.isneginf(gold["bad_words"][:, 85]).all()      # [eos] dropped
    assert np.isneginf(gold["bad_words"][[0, 2], 86]).all() and np.isfinite(gold["bad_words"][1, 86])
    assert same(R.forced_eos(x, 4, 5, C.FORCED), gold["forced_eos_last"]) and same(R.forced_eos(x, 4, 8, C.FORCED), gold["forced_eos_before"])
    assert same(R.exponential_decay(x, 4, C.EOS, *C.DECAY), gold["exponential_decay"])
    assert same(R.exponential_decay(x, 4, C.EOS, 4, C.DECAY[1]), gold["exponential_decay_before"]) and same(gold["exponential_decay_before"], x)
    assert same(R.suppress(x, C.SUPPRESS), gold["suppress"])
    assert same(R.begin_suppress(x, 0, C.BEGIN_SUPPRESS), gold["begin_suppress_t0"])
    assert same(R.begin_suppress(x, 4, C.BEGIN_SUPPRESS), gold["begin_suppress_t4"])


def test_all_processors_together_match_hfs_own_list(gold):
    order = json.loads(bytes(gold["hf_order_json"]).decode())
    assert order["processors"] == ["SequenceBiasLogitsProcessor", "RepetitionPenaltyLogitsProcessor", "NoRepeatNGramLogitsProcessor",
                                   "NoBadWordsLogitsProcessor", "MinNewTokensLengthLogitsProcessor", "ForcedEOSTokenLogitsProcessor",
                                   "ExponentialDecayLengthPenalty", "SuppressTokensLogitsProcessor", "SuppressTokensAtBeginLogitsProcessor"]
    assert order["with_do_sample"] == order["processors"] + ["TemperatureLogitsWarper", "TopKLogitsWarper", "TopPLogitsWarper",
                                                              "MinPLogitsWarper", "TypicalLogitsWarper", "EpsilonLogitsWarper",
                                                              "EtaLogitsWarper", "LogitNormalization"]
    x, ctx = gold["scores"], gold["context"]
    seen = set()
    for tag, t, max_new in C.CHAIN_POINTS:
        kw = C.chain_generation_kwargs(max_new)
        got = R.process(x, ctx[:, :C.L + t], t, max_new, C.V, sequence_bias_entries=kw["sequence_bias"],
                        repetition_penalty=kw["repetition_penalty"], no_repeat_ngram_size=kw["no_repeat_ngram_size"],
                        bad_words_ids=kw["bad_words_ids"], min_new_tokens=kw["min_new_tokens"], eos_ids=C.EOS, forced_eos_ids=C.FORCED,
                        exponential_decay_length_penalty=C.DECAY, suppress_tokens=C.SUPPRESS, begin_suppress_tokens=C.BEGIN_SUPPRESS)
        assert same(got, gold[f"chain_{tag}"]), tag
        seen.add(gold[f"chain_{tag}"].tobytes())
    assert len(seen) == 3                                           # the three points differ: every step-indexed rule fired somewhere


def test_float64_warpers_agree_with_hf_outside_the_bands(gold):
    x = gold["scores"]
    bands = {k[5:]: float(gold[k]) for k in gold if k.startswith("band_")}
    assert set(bands) == {"min_p", "epsilon", "eta", "typical_s", "typical_mass"} and all(1e-5 <= b < 1e-3 for b in bands.values())
    for name, kw in (("min_p", dict(min_p_value=C.MIN_P)), ("typical_p", dict(typical_p=C.TYPICAL_P)),
                     ("epsilon_cutoff", dict(eps=C.EPSILON)), ("eta_cutoff", dict(eta=C.ETA))):
        ref, und = R.warp_ext(x, **kw, bands=bands)
        R.check_warp(gold[name], x, ref, und, C.V)
        assert np.isneginf(ref).any() and not np.isneginf(ref).all(axis=1).any(), name


def test_warper_reference_edge_rows():
    x = np.full((2, 50), -np.inf, np.float32)
    x[0, 17], x[1, 3], x[1, 4] = 1.5, 2.0, 2.0
    for kw in (dict(min_p_value=0.5), dict(typical_p=0.5), dict(eps=0.3), dict(eta=0.3)):
        ref, _ = R.warp_ext(x, **kw)
        assert same(ref, x), kw                                     # one survivor / two tied survivors: nothing to remove
    y = np.zeros((1, 8), np.float32)
    y[0, :4] = 3.0                                                  # four tied maxima and four tied others
    ref, _ = R.warp_ext(y, typical_p=0.5)
    assert np.isfinite(ref[0, :4]).all() or np.isfinite(ref[0, 4:]).all()      # a tied group survives or falls as a whole
    assert len(set(np.isfinite(ref[0, :4]))) == 1 and len(set(np.isfinite(ref[0, 4:]))) == 1


# ----------------------------------------------------------------------------- the table builder
def test_sequence_table_order_inside_a_group():
    entries = ops.normalize_sequence_bias(dict(C.SEQUENCE_BIAS))
    assert entries == [(tuple(k), float(v)) for k, v in C.SEQUENCE_BIAS]
    tab = ops.build_sequence_table(entries, C.V)
    toks, offs, bias, groups = (tab[k].tolist() for k in ("tokens", "offsets", "bias", "groups"))
    seqs = [tuple(toks[offs[i]:offs[i + 1]]) for i in range(tab["n_seq"])]
    assert tab["n_seq"] == len(entries) == len(bias) and tab["n_tokens"] == len(toks) == offs[-1] and tab["n_groups"] == len(groups) - 1
    lasts = [s[-1] for s in seqs]
    assert lasts == sorted(lasts) and groups[0] == 0 and groups[-1] == len(seqs)
    assert [lasts[g] for g in groups[:-1]] == sorted(set(lasts))     # one group per last token
    g60 = seqs[lasts.index(60):lasts.index(60) + 3]
    assert g60 == [(60,), (41, 60), (40, 41, 60)] and bias[lasts.index(60):lasts.index(60) + 3] == [1e8, -1e8, 1.0]
    # the length-1 entry goes first whatever its place in the input (HF adds its length-1 row first), the rest keep the given order
    tab = ops.build_sequence_table([((9, 5), 1.0), ((8, 5), 2.0), ((5,), 3.0), ((7, 8, 5), 4.0), ((2,), 5.0)], 10)
    assert tab["tokens"].tolist() == [2, 5, 9, 5, 8, 5, 7, 8, 5] and tab["bias"].tolist() == [5.0, 3.0, 1.0, 2.0, 4.0]
    assert tab["groups"].tolist() == [0, 1, 5] and tab["offsets"].dtype == torch.int32 and tab["tokens"].dtype == torch.int64
    assert ops.build_sequence_table([], 10) is None


def test_both_sequence_bias_forms_and_bad_word_filtering():
    d = {(5,): 1.0, (4, 5): -2.0}
    assert ops.normalize_sequence_bias(d) == ops.normalize_sequence_bias([[[5], 1.0], [[4, 5], -2.0]]) == [((5,), 1.0), ((4, 5), -2.0)]
    assert ops.normalize_sequence_bias([[[5], 1.0], [[5], 3.0]]) == [((5,), 3.0)]            # the list form becomes a dict, as in HF
    assert ops.normalize_bad_words([[7], [3, 7], [11], [9], [9]], eos_ids=(7, 11)) == [((3, 7), -np.inf), ((9,), -np.inf)]
    assert ops.normalize_bad_words([[7]], eos_ids=(7,)) == []


# ----------------------------------------------------------------------------- errors
@pytest.mark.parametrize("bad, match", [
    ({}, "non-empty"), ([], "non-empty"), ("x", "non-empty"), ({5: 1.0}, "tuples as keys"), ({(): 1.0}, "non-empty tuple"),
    ({(-1,): 1.0}, "positive integers"), ({(1.5,): 1.0}, "positive integers"), ({(5,): 1}, "floats as values"),
    ([[[5], 1]], "lists of positive integers and float"), ([[5, 1.0]], "lists of positive integers and float"),
    ([[[0], 1.0]], "lists of positive integers and float"), ([[[], 1.0]], "lists of positive integers and float")])
def test_malformed_sequence_bias_raises_hfs_errors(bad, match):
    with pytest.raises(ValueError, match=match):
        ops.normalize_sequence_bias(bad)


def test_table_and_argument_errors():
    with pytest.raises(ValueError, match="vocabulary size is 100, but the following tokens were being biased: \\[100\\]"):
        ops.build_sequence_table([((3, 100), 1.0)], 100)
    with pytest.raises(ValueError, match=f"limit of {ops.SEQ_BIAS_MAX_SEQS}"):
        ops.build_sequence_table([((i // 90 + 1, i % 90), 1.0) for i in range(ops.SEQ_BIAS_MAX_SEQS + 1)], 100)
    with pytest.raises(ValueError, match=f"limit of {ops.SEQ_BIAS_MAX_LEN}"):
        ops.build_sequence_table([(tuple(range(ops.SEQ_BIAS_MAX_LEN + 1)), 1.0)], 100)
    assert ops.SEQ_BIAS_MAX_SEQS >= 1024 and ops.SEQ_BIAS_MAX_LEN >= 32
    text = open(_lib.HEADER).read()
    assert f"#define TA_SEQ_BIAS_MAX_SEQS {ops.SEQ_BIAS_MAX_SEQS}" in text and f"#define TA_SEQ_BIAS_MAX_LEN {ops.SEQ_BIAS_MAX_LEN}" in text
    ops.build_sequence_table([((i // 90 + 1, i % 90), 1.0) for i in range(1024)] + [(tuple(range(1, 33)), 1.0)], 100)      # the promised size
    for bad, match in (([], "non-empty list"), ("x", "non-empty list"), ([5], "list of lists"), ([[-1]], "positive integers")):
        with pytest.raises(ValueError, match=match):
            ops.normalize_bad_words(bad)
    for kw, match in ((dict(min_p=1.5), "`min_p` has to be a float in the \\[0, 1\\] interval"), (dict(min_p=-0.1), "`min_p`"),
                      (dict(typical_p=0.0), "`typical_p` has to be a float > 0 and < 1"), (dict(typical_p=1.5), "`typical_p`"),
                      (dict(epsilon_cutoff=1.0), "`epsilon_cutoff` has to be a float > 0 and < 1"), (dict(epsilon_cutoff=-1e-3), "`epsilon_cutoff`"),
                      (dict(eta_cutoff=1.0), "`eta_cutoff` has to be a float > 0 and < 1"), (dict(eta_cutoff=-1e-3), "`eta_cutoff`")):
        with pytest.raises(ValueError, match=match):
            ops.check_warp_ext(**kw)
    assert ops.check_warp_ext() == (0.0, 1.0, 0.0, 0.0) and ops.check_warp_ext(0.05, 0.9, 3e-4, 2e-3) == (0.05, 0.9, 3e-4, 2e-3)
    with pytest.raises(ValueError, match="vocabulary size is 100"):
        ops.id_list([3, 100], 100, "suppress_tokens")
    start, m = ops.decay_multipliers((2, 1.5), 6)
    assert start == 2 and m.dtype == torch.float32 and m.tolist() == [0.0, 0.0, 0.0] + [float(R.decay_multiplier(t, 2, 1.5)) for t in (3, 4, 5)]


# ----------------------------------------------------------------------------- dry-run plumbing through generate
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


STEP = ("ta_logits_sequence_bias", "ta_logits_process", "ta_logits_suppress_until", "ta_logits_step_rules", "ta_logits_warp",
        "ta_logits_warp_ext", "ta_sample_f32", "ta_argmax_f32", "ta_token_scores_f32", "ta_greedy_advance")


def _step_calls(dry):
    return [c for c in dry.calls if c in STEP]


def test_no_option_launches_what_the_parent_launched(dry):
    m, kw = _model()
    dry.calls.clear()
    out = m.generate(**kw, max_new_tokens=4, eos_token_id=[])
    assert _step_calls(dry) == ["ta_argmax_f32", "ta_greedy_advance"] * 4 and out.shape == (2, 4)
    dry.calls.clear()
    m.generate(**kw, max_new_tokens=3, eos_token_id=[991], repetition_penalty=1.2, min_new_tokens=2, do_sample=True, top_k=5, seed=1,
               renormalize_logits=True)
    assert _step_calls(dry) == ["ta_logits_process", "ta_logits_suppress_until", "ta_logits_warp", "ta_sample_f32", "ta_greedy_advance"] * 3
    # the warpers act under do_sample only, as in HF
    dry.calls.clear()
    m.generate(**kw, max_new_tokens=3, eos_token_id=[], min_p=0.1, typical_p=0.9, epsilon_cutoff=1e-3, eta_cutoff=1e-3)
    assert _step_calls(dry) == ["ta_argmax_f32", "ta_greedy_advance"] * 3
    # off values launch nothing either
    dry.calls.clear()
    m.generate(**kw, max_new_tokens=3, eos_token_id=[], do_sample=True, seed=1, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0,
               bad_words_ids=None, suppress_tokens=[])
    assert _step_calls(dry) == ["ta_logits_warp", "ta_sample_f32", "ta_greedy_advance"] * 3


@pytest.mark.parametrize("option, expect", [
    (dict(sequence_bias={(5,): 2.0}), ["ta_logits_sequence_bias", "ta_logits_process"]),
    (dict(sequence_bias=[[[5, 6], 2.0]]), ["ta_logits_sequence_bias", "ta_logits_process"]),
    (dict(bad_words_ids=[[5], [6, 7]]), ["ta_logits_process", "ta_logits_sequence_bias"]),
    (dict(forced_eos_token_id=991), ["ta_logits_process", "ta_logits_step_rules"]),
    (dict(exponential_decay_length_penalty=(2, 1.5)), ["ta_logits_process", "ta_logits_step_rules"]),
    (dict(suppress_tokens=[1, 2]), ["ta_logits_process", "ta_logits_step_rules"]),
    (dict(begin_suppress_tokens=[1, 2]), ["ta_logits_process", "ta_logits_step_rules"])])
def test_each_option_sits_at_hfs_place(dry, option, expect):
    m, kw = _model()
    dry.calls.clear()
    m.generate(**kw, max_new_tokens=3, eos_token_id=[991], repetition_penalty=1.2, **option)
    assert _step_calls(dry) == (expect + ["ta_argmax_f32", "ta_greedy_advance"]) * 3
    assert dry.calls.count("ta_lm_decode_step") == 2


@pytest.mark.parametrize("option", [dict(min_p=0.1), dict(typical_p=0.9), dict(epsilon_cutoff=1e-3), dict(eta_cutoff=1e-3)])
def test_each_warper_follows_ta_logits_warp(dry, option):
    m, kw = _model()
    dry.calls.clear()
    m.generate(**kw, max_new_tokens=3, eos_token_id=[], do_sample=True, top_k=5, seed=3, **option)
    assert _step_calls(dry) == ["ta_logits_warp", "ta_logits_warp_ext", "ta_sample_f32", "ta_greedy_advance"] * 3


def test_everything_together_is_hfs_order_and_config_is_read(dry):
    m, kw = _model()
    m.config.suppress_tokens = [1, 2]                               # the generation config is the second source, the call the first
    m.config.bad_words_ids = [[3]]
    dry.calls.clear()
    m.generate(**kw, max_new_tokens=3, eos_token_id=[991], sequence_bias={(5,): 2.0}, repetition_penalty=1.2, no_repeat_ngram_size=2,
               min_new_tokens=1, forced_eos_token_id=[991], exponential_decay_length_penalty=(1, 1.1), begin_suppress_tokens=[4],
               do_sample=True, temperature=0.7, top_k=20, top_p=0.9, min_p=0.05, typical_p=0.9, epsilon_cutoff=3e-4, eta_cutoff=2e-3,
               renormalize_logits=True, seed=5, return_token_scores=True)
    assert _step_calls(dry) == ["ta_logits_sequence_bias", "ta_logits_process", "ta_logits_sequence_bias", "ta_logits_suppress_until",
                                "ta_logits_step_rules", "ta_logits_warp", "ta_logits_warp_ext", "ta_sample_f32", "ta_token_scores_f32",
                                "ta_greedy_advance"] * 3
    dry.calls.clear()
    m.generate(**kw, max_new_tokens=2, eos_token_id=[], bad_words_ids=[[991]], suppress_tokens=[])      # the call overrides the config
    assert _step_calls(dry) == ["ta_logits_sequence_bias", "ta_argmax_f32", "ta_greedy_advance"] * 2
    dry.calls.clear()
    m.generate(**kw, max_new_tokens=2, eos_token_id=[991], bad_words_ids=[[991]], suppress_tokens=[])   # [eos] only: dropped, nothing left
    assert _step_calls(dry) == ["ta_argmax_f32", "ta_greedy_advance"] * 2
    # streaming: the same launches
    one = dict(input_features=kw["input_features"][:1], audio_attention_mask=kw["audio_attention_mask"][:1], input_ids=kw["input_ids"][:1])
    dry.calls.clear()
    got = list(m.generate_streaming(**one, return_token_ids=True, max_new_tokens=3, eos_token_id=[], bad_words_ids=[[8, 5]],
                                    suppress_tokens=[7]))
    assert len(got) == 3 and _step_calls(dry) == ["ta_logits_sequence_bias", "ta_logits_step_rules", "ta_argmax_f32", "ta_greedy_advance"] * 3


def test_generate_errors(dry):
    m, kw = _model()
    g = lambda **o: m.generate(**kw, max_new_tokens=3, eos_token_id=[991], **o)  # noqa: E731
    for o, match in ((dict(bad_words_ids=[[1000]]), "vocabulary size is 1000"), (dict(sequence_bias={(1000,): 1.0}), "vocabulary size is 1000"),
                     (dict(suppress_tokens=[1000]), "vocabulary size is 1000"), (dict(begin_suppress_tokens=[-1]), "vocabulary size is 1000"),
                     (dict(forced_eos_token_id=1000), "vocabulary size is 1000"), (dict(sequence_bias={5: 1.0}), "tuples as keys"),
                     (dict(min_p=2.0), "`min_p`"), (dict(typical_p=0.0), "`typical_p`"), (dict(epsilon_cutoff=1.0), "`epsilon_cutoff`"),
                     (dict(eta_cutoff=1.0), "`eta_cutoff`"),
                     (dict(bad_words_ids=[[i % 900 + 1, i // 900 + 1] for i in range(4097)]), "limit of 4096"),
                     (dict(bad_words_ids=[list(range(1, 40))]), "limit of 32"),
                     (dict(min_new_tokens=3, exponential_decay_length_penalty=(2, 1.5)), "NaN"),
                     (dict(exponential_decay_length_penalty=(2,)), "pair")):
        with pytest.raises(ValueError, match=match):
            g(**o)
    with pytest.raises(NotImplementedError):
        g(num_beams=2, bad_words_ids=[[5]])
    # without eos ids the length penalty has nothing to act on, as in HF: no launch, no error
    dry.calls.clear()
    m.generate(**kw, max_new_tokens=2, eos_token_id=[], min_new_tokens=2, exponential_decay_length_penalty=(1, 1.5))
    assert dry.calls.count("ta_logits_step_rules") == 0


# ----------------------------------------------------------------------------- operators and wrappers
def test_operators_are_registered_and_wrappers_validate(dry):
    from tiny_audio_amd import torch_ops
    assert {"logits_sequence_bias", "logits_step_rules", "logits_warp_ext"} <= set(torch_ops.OPERATORS)
    s = str(torch.ops.ta355.logits_warp_ext.default._schema)
    assert s.startswith("ta355::logits_warp_ext(Tensor(a0!) logits, SymInt V, float min_p, float typical_p, float epsilon_cutoff, float eta_cutoff) -> ()"), s
    assert "Tensor(a0!) logits" in str(torch.ops.ta355.logits_sequence_bias.default._schema)
    assert "Tensor(a0!) logits" in str(torch.ops.ta355.logits_step_rules.default._schema)
    x, ctx = torch.zeros(3, 128), torch.zeros(3, 6, dtype=torch.int64)
    dry.calls.clear()
    assert ops.logits_sequence_bias(x, 100, ctx, [((5,), 1.0), ((0, 5), 2.0)]) is x
    assert ops.logits_sequence_bias(x, 100, ctx[:, :0], [((5,), 1.0)]) is x and ops.logits_sequence_bias(x, 100, ctx, []) is x
    assert ops.logits_step_rules(x, 100, 0, 4, forced_eos_ids=[7], eos_ids=[7], exponential_decay_length_penalty=(1, 1.5),
                                 suppress_tokens=[1], begin_suppress_tokens=[2]) is x
    assert ops.logits_warp_ext(x[:, :120], 100, min_p=0.1) is not None
    tab = ops.build_sequence_table([((5,), 1.0)], 100)
    torch.ops.ta355.logits_sequence_bias(x, 100, ctx, tab["tokens"], tab["offsets"], tab["bias"], tab["groups"])
    torch.ops.ta355.logits_step_rules(x, 100, 1, 4, [7], [7], 1, 1.5, [], [2])
    torch.ops.ta355.logits_warp_ext(x, 100, 0.0, 0.9, 0.0, 0.0)
    assert dry.calls == ["ta_logits_sequence_bias"] * 2 + ["ta_logits_step_rules", "ta_logits_warp_ext", "ta_logits_sequence_bias",
                                                           "ta_logits_step_rules", "ta_logits_warp_ext"]
    for bad in (lambda: ops.logits_warp_ext(x.double(), 100, min_p=0.1), lambda: ops.logits_warp_ext(x, 129, min_p=0.1),
                lambda: ops.logits_warp_ext(x, 100, min_p=1.1), lambda: ops.logits_step_rules(x, 100, 4, 4, suppress_tokens=[1]),
                lambda: ops.logits_step_rules(x, 100, 0, 4, suppress_tokens=[100]), lambda: ops.logits_sequence_bias(x, 100, ctx.int(), [((5,), 1.0)]),
                lambda: ops.logits_sequence_bias(x, 100, ctx[:2], [((5,), 1.0)]), lambda: ops.logits_sequence_bias(x, 100, ctx, [((100,), 1.0)])):
        with pytest.raises(ValueError):
            bad()


def test_header_declares_the_entry_points_and_the_abi_version_stays():
    protos = _lib.parse_header()
    assert len(protos["ta_logits_sequence_bias"][1]) == 17 and len(protos["ta_logits_step_rules"][1]) == 17
    assert len(protos["ta_logits_warp_ext"][1]) == 9
    assert _lib.lib().ta_version() == 4
    text = open(_lib.HEADER).read()
    for cls in ("SequenceBiasLogitsProcessor", "NoBadWordsLogitsProcessor", "ForcedEOSTokenLogitsProcessor", "ExponentialDecayLengthPenalty",
                "SuppressTokensLogitsProcessor", "SuppressTokensAtBeginLogitsProcessor", "MinPLogitsWarper", "TypicalLogitsWarper",
                "EpsilonLogitsWarper", "EtaLogitsWarper"):
        assert cls in text, cls

"""The decoding drivers (``tiny_audio_amd/decoding.py``) without a GPU: the COMPLETE dry-run launch list of every driver, unfiltered and in
order, against lists recorded from the drivers as they stood before the prompt pass, the processor chain and the step loop were made
single pieces; and the step loop's schedule against the rule it restates."""
import pytest
import torch

from oracle import weights as OW
from tiny_audio_amd import scoring
from tests.test_decode_options_host import dry  # noqa: F401


def _model(lora=False):
    """tests/test_decode_options_host.py::_model (vocab 1000, two LM layers, B = 2, L = 16), optionally with adapters"""
    from tiny_audio_amd.asr_config import ASRConfig
    from tiny_audio_amd.asr_modeling import ASRModel
    enc, lm = OW.enc_config(hidden=256, ffn=512, layers=1, heads=4), OW.lm_config(vocab=1000, hidden=256, ffn=512, layers=2, heads=4, kv_heads=2)
    cfg = ASRConfig(audio_config=enc, text_config=lm, projector_hidden_dim=128, audio_token_id=999, pad_token_id=990, eos_token_id=991,
                    use_lora=lora)
    m = ASRModel(cfg, device="cpu", init="random")
    ids = torch.tensor([[5, 6] + [999] * 12 + [7, 8]] * 2)
    kw = dict(input_ids=ids, input_features=torch.zeros(2, 128, 100), audio_attention_mask=torch.ones(2, 100, dtype=torch.int64),
              attention_mask=torch.ones_like(ids))
    return m, kw


def _everything(m, kw):
    m.config.suppress_tokens = [1, 2]
    m.config.bad_words_ids = [[3]]
    m.generate(**kw, max_new_tokens=3, eos_token_id=[991], sequence_bias={(5,): 2.0}, repetition_penalty=1.2, no_repeat_ngram_size=2,
               min_new_tokens=1, forced_eos_token_id=[991], exponential_decay_length_penalty=(1, 1.1), begin_suppress_tokens=[4],
               do_sample=True, temperature=0.7, top_k=20, top_p=0.9, min_p=0.05, typical_p=0.9, epsilon_cutoff=3e-4, eta_cutoff=2e-3,
               renormalize_logits=True, seed=5, return_token_scores=True)


def _streaming(m, kw):
    one = dict(input_features=kw["input_features"][:1], audio_attention_mask=kw["audio_attention_mask"][:1], input_ids=kw["input_ids"][:1])
    got = list(m.generate_streaming(**one, return_token_ids=True, return_token_scores=True, max_new_tokens=3, eos_token_id=[],
                                    repetition_penalty=1.2, bad_words_ids=[[8, 5]]))
    assert len(got) == 3 and all(isinstance(t, int) and isinstance(lp, float) for t, lp in got)


def _beams(trace, K=3):
    def run(m, kw):
        out = m.generate_beams(**kw, max_new_tokens=4, eos_token_id=[991], num_beams=K, return_beam_trace=trace, sequence_bias={(5,): 2.0},
                               repetition_penalty=1.2, no_repeat_ngram_size=2, bad_words_ids=[[6, 7]], min_new_tokens=1,
                               forced_eos_token_id=[991], exponential_decay_length_penalty=(1, 1.1), suppress_tokens=[1],
                               begin_suppress_tokens=[4])
        assert isinstance(out, tuple) == trace
    return run


def _score_three_chunks(m, kw):
    tab = scoring.build_candidate_table([[[1]] * 3, [[2, 3]] * 2], None, 991, False, max_rows=2)
    assert len(tab["chunks"]) == 3
    a = m._prepare_generation(kw["input_ids"], kw["input_features"], kw["audio_attention_mask"], kw["attention_mask"], None, {})
    m.language_model.score_candidates(a["input_ids"], a["src_row"], a["audio"], a["attention_mask"], tab["token_ids"], tab["n_tokens"],
                                      tab["candidate_clip"], tab["chunks"])


def _score_nothing(m, kw):
    out = m.score(kw["input_features"], kw["audio_attention_mask"], [[], []], input_ids=kw["input_ids"], attention_mask=kw["attention_mask"])
    assert out.scores.shape == (0,)


# name -> (with adapters, the call)
CASES = {
    "generate": (False, lambda m, kw: m.generate(**kw, max_new_tokens=5, eos_token_id=[])),
    "generate_lora": (True, lambda m, kw: m.generate(**kw, max_new_tokens=5, eos_token_id=[])),
    "everything": (False, _everything),
    "streaming": (False, _streaming),
    "beams_trace": (False, _beams(True)),
    "beams": (False, _beams(False)),
    "one_beam": (False, lambda m, kw: m.generate_beams(**kw, max_new_tokens=4, eos_token_id=[991], num_beams=1)),
    "score_three_chunks": (False, _score_three_chunks),
    "generate_nothing": (False, lambda m, kw: m.generate(**kw, max_new_tokens=0, eos_token_id=[])),
    "beams_nothing": (False, lambda m, kw: m.generate_beams(**kw, max_new_tokens=0, eos_token_id=[991], num_beams=3)),
    "score_nothing": (False, _score_nothing),
}

# recorded from the three drivers of language_model.py before they were composed of shared pieces
AUDIO = ["ta_encoder_forward", "ta_cast_f32_bf16", "ta_cast_f32_bf16", "ta_transpose_to_bf16", "ta_mlp_projector_forward", "ta_audio_index"]
CHAIN = ["ta_logits_sequence_bias", "ta_logits_process", "ta_logits_sequence_bias", "ta_logits_suppress_until", "ta_logits_step_rules"]
DECODE = ["ta_lm_decode_step"]


def _steps(n, block):
    """the prompt pass's selection, then n - 1 decode steps with the same one"""
    return block + (DECODE + block) * (n - 1)


GREEDY = ["ta_argmax_f32", "ta_greedy_advance"]
SAMPLED = CHAIN + ["ta_logits_warp", "ta_logits_warp_ext", "ta_sample_f32", "ta_token_scores_f32", "ta_greedy_advance"]
STREAMED = ["ta_logits_process", "ta_logits_sequence_bias", "ta_argmax_f32", "ta_token_scores_f32", "ta_greedy_advance"]
BEAMS = ["ta_beam_logprobs_f32"] + CHAIN + ["ta_beam_topk_f32", "ta_beam_advance", "ta_kv_beam_reorder"]
ONE_BEAM = ["ta_beam_logprobs_f32", "ta_beam_topk_f32", "ta_beam_advance"]
EXPECT = {
    "generate": AUDIO + ["ta_lm_prefill"] + _steps(5, GREEDY),
    "generate_lora": AUDIO + ["ta_lm_prefill"] + _steps(5, GREEDY),
    "everything": AUDIO + ["ta_lm_prefill"] + _steps(3, SAMPLED),
    "streaming": AUDIO + ["ta_lm_prefill"] + _steps(3, STREAMED),
    "beams_trace": AUDIO + ["ta_lm_prefill", "ta_kv_beam_expand"] + _steps(4, BEAMS),
    "beams": AUDIO + ["ta_lm_prefill", "ta_kv_beam_expand"] + _steps(4, BEAMS),
    "one_beam": AUDIO + ["ta_lm_prefill", "ta_kv_beam_expand"] + _steps(4, ONE_BEAM),
    "score_three_chunks": AUDIO + ["ta_lm_prefill"] + ["ta_lm_score"] * 3,
    "generate_nothing": AUDIO,
    "beams_nothing": AUDIO,
    "score_nothing": AUDIO,
}


@pytest.mark.parametrize("name", list(CASES))
def test_complete_launch_list_is_the_recorded_one(dry, name):  # noqa: F811
    lora, call = CASES[name]
    m, kw = _model(lora)
    dry.calls.clear()
    call(m, kw)
    assert dry.calls == EXPECT[name]


def test_streaming_restores_the_training_mode_when_closed_early(dry):  # noqa: F811
    m, kw = _model()
    one = dict(input_features=kw["input_features"][:1], audio_attention_mask=kw["audio_attention_mask"][:1], input_ids=kw["input_ids"][:1])
    m.train()
    g = m.generate_streaming(**one, return_token_ids=True, max_new_tokens=3, eos_token_id=[])
    next(g)
    assert not m.training
    g.close()
    assert m.training
    with pytest.raises(ValueError, match="vocabulary size is 1000"):
        m.generate(**kw, max_new_tokens=3, suppress_tokens=[1000])
    assert m.training


# ----------------------------------------------------------------------------- the step loop alone
def _expected_steps(max_new, sync_every, every_step, s):
    """The schedule of the drivers' loops, restated: for t in 1..max_new-1, before step t the counter is read if ``every_step`` or
    t % sync_every == 0, and the loop stops there if it reads 0; the counter drops to 0 during the s-th step."""
    n = 0
    for t in range(1, max_new):
        if (every_step or t % sync_every == 0) and n >= s:
            break
        n += 1
    return n


@pytest.mark.parametrize("sync_every", [1, 8])
@pytest.mark.parametrize("every_step", [False, True])
@pytest.mark.parametrize("s", [1, 7, 8, 9])
def test_step_loop_schedule(sync_every, every_step, s, monkeypatch):
    from tiny_audio_amd.decoding import step_loop

    def no_graph(*a, **k):
        raise AssertionError("the step loop must not capture a graph on the CPU")
    monkeypatch.setattr(torch.cuda, "CUDAGraph", no_graph)
    monkeypatch.setattr(torch.cuda, "graph", no_graph)
    alive, ran = torch.ones(1, dtype=torch.int32), []

    def step():
        ran.append(1)
        if len(ran) == s:
            alive.zero_()

    ts = list(step_loop(step, 20, alive, sync_every, every_step, True, torch.device("cpu")))
    want = _expected_steps(20, sync_every, every_step, s)
    # every executed step is a direct call of ``step``: on the CPU nothing is captured or replayed, ``use_graph`` or not
    assert len(ran) == want and ts == list(range(1, want + 1))
    assert want == {(1, False): s, (1, True): s, (8, True): s, (8, False): 7 if s <= 7 else 15}[(sync_every, every_step)]

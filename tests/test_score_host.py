"""Candidate scoring, host side (no GPU): ``scoring.build_candidate_table`` / ``chunk_rows`` / ``pick``, ``ScoreOutput``, and every
TA_ERR_ARG refusal of ``ta_attention_extend`` and ``ta_lm_score`` through the C ABI -- each is decided before the first HIP call, so the
fake (never dereferenced) device pointers below are safe."""
import ctypes as C

import pytest
import torch

from tiny_audio_amd import scoring


class ToyTokenizer:
    """Whitespace words -> ids 10 + index in WORDS; an unknown word is dropped (so a text of unknown words tokenises to nothing)."""
    WORDS = ("yes", "no", "maybe", "the", "cat", "sat")

    def __len__(self):
        return 64

    def __call__(self, text, add_special_tokens=True):
        assert add_special_tokens is False
        return {"input_ids": [10 + self.WORDS.index(w) for w in text.split() if w in self.WORDS]}


EOS = 3


# ============================================================================ build_candidate_table
def test_table_ragged_mixed_and_an_empty_clip():
    t = scoring.build_candidate_table([["yes", [7, 8, 9]], [], ["the cat sat"]], ToyTokenizer(), EOS, append_eos=True)
    assert t["token_ids"].tolist() == [[10, 3, 0, 0], [7, 8, 9, 3], [13, 14, 15, 3]]
    assert t["n_tokens"].tolist() == [2, 4, 4] and t["candidate_clip"].tolist() == [0, 0, 2] and t["n_clips"] == 3
    assert t["token_ids"].dtype == t["n_tokens"].dtype == t["candidate_clip"].dtype == torch.int64
    assert t["chunks"] == [(0, 3)]


def test_table_without_eos_and_tensor_entries():
    t = scoring.build_candidate_table([[torch.tensor([5, 6]), "no"]], ToyTokenizer(), EOS, append_eos=False)
    assert t["token_ids"].tolist() == [[5, 6], [11, 0]] and t["n_tokens"].tolist() == [2, 1]


def test_table_no_candidates_at_all():
    t = scoring.build_candidate_table([[], []], None, EOS, append_eos=True)
    assert t["token_ids"].shape == (0, 0) and t["n_tokens"].numel() == 0 and t["chunks"] == [] and t["n_clips"] == 2


@pytest.mark.parametrize("cands, what", [([["zebra"]], "empty after tokenisation"), ([[[]]], "empty after tokenisation"),
                                         ([[[5, 64]]], "outside the vocabulary"), ([[[-1]]], "outside the vocabulary")])
def test_table_refusals(cands, what):
    with pytest.raises(ValueError, match=what):
        scoring.build_candidate_table(cands, ToyTokenizer(), EOS, append_eos=True)


def test_table_eos_outside_the_vocabulary_and_strings_without_tokenizer():
    with pytest.raises(ValueError, match="outside the vocabulary"):
        scoring.build_candidate_table([[[5]]], ToyTokenizer(), 64, append_eos=True)
    with pytest.raises(ValueError, match="no tokenizer"):
        scoring.build_candidate_table([["yes"]], None, EOS, append_eos=True)


def test_chunking_at_the_row_and_cell_limits():
    max_r, max_t, max_c = scoring.limits()
    assert (max_r, max_t, max_c) == (1024, 256, 65536)
    assert scoring.chunk_rows([1] * 1024, max_r, max_t, max_c) == [(0, 1024)]
    assert scoring.chunk_rows([1] * 1025, max_r, max_t, max_c) == [(0, 1024), (1024, 1025)]
    # rows * longest row: 256 rows of 256 tokens fill a call, one more row starts the next
    assert scoring.chunk_rows([256] * 257, max_r, max_t, max_c) == [(0, 256), (256, 257)]
    # a long row arriving late counts for the rows already in the chunk
    assert scoring.chunk_rows([1, 1, 1, 4], 8, 4, 12) == [(0, 3), (3, 4)]
    assert scoring.chunk_rows([1, 1, 4], 8, 4, 12) == [(0, 3)]
    assert scoring.chunk_rows([], 8, 4, 12) == []
    with pytest.raises(ValueError, match="at most 256"):
        scoring.chunk_rows([257], max_r, max_t, max_c)
    t = scoring.build_candidate_table([[[1]] * 5], None, EOS, append_eos=False, max_rows=2)
    assert t["chunks"] == [(0, 2), (2, 4), (4, 5)]


# ============================================================================ pick / ScoreOutput
def test_pick_tie_rule_and_both_normalisations():
    scores = torch.tensor([-4.0, -2.0, -2.0, -9.0, -1.0, -6.0])
    n_tok = torch.tensor([1, 2, 1, 3, 1, 2])
    clip = torch.tensor([0, 0, 0, 2, 2, 2])
    assert scoring.pick(scores, n_tok, clip) == [1, -1, 1]                  # the tie between candidates 1 and 2 of clip 0: the lower index
    assert scoring.pick(scores, n_tok, clip, normalize="mean") == [1, -1, 1]   # clip 0: -4, -1, -2; clip 2: -3, -1, -3
    assert scoring.pick(torch.tensor([-4.0, -6.0]), torch.tensor([1, 3]), torch.tensor([0, 0]), normalize="mean") == [1]
    assert scoring.pick(torch.tensor([-4.0, -6.0]), torch.tensor([1, 3]), torch.tensor([0, 0]), normalize="sum") == [0]
    assert scoring.pick(scores, n_tok, clip, n_clips=4) == [1, -1, 1, -1]
    assert scoring.pick(torch.zeros(0), torch.zeros(0), torch.zeros(0, dtype=torch.int64)) == []
    with pytest.raises(ValueError):
        scoring.pick(scores, n_tok, clip, normalize="max")


def test_score_output_access_and_per_clip():
    from tiny_audio_amd.asr_modeling import ScoreOutput
    o = ScoreOutput(scores=torch.tensor([-1.0, -2.0, -3.0]), candidate_clip=torch.tensor([0, 0, 2]), n_tokens=torch.tensor([1, 2, 1]),
                    token_ids=torch.tensor([[4, 0], [5, 6], [7, 0]]), token_logprobs=torch.tensor([[-1.0, 0.0], [-0.5, -1.5], [-3.0, 0.0]]),
                    n_clips=3)
    assert list(o) == ["scores", "candidate_clip", "n_tokens", "token_ids", "token_logprobs"]
    assert o.scores is o["scores"] is o[0] and len(o[:2]) == 2
    pc = o.per_clip()
    assert [len(c) for c in pc] == [2, 0, 1]
    assert pc[0][1] == dict(score=-2.0, n_tokens=2, token_ids=[5, 6], token_logprobs=[-0.5, -1.5])
    bare = ScoreOutput(scores=o.scores, candidate_clip=o.candidate_clip, n_tokens=o.n_tokens, n_clips=3)
    assert bare.token_logprobs is None and "token_ids" not in bare and bare.per_clip()[2] == [dict(score=-3.0, n_tokens=1)]
    with pytest.raises(AttributeError):
        bare.nothing


def test_rescore_cuts_every_hypothesis_behind_its_first_eos():
    class Model:
        class config:
            eos_token_id, pad_token_id = 3, 0

        def score(self, feats, amask, cands, **kw):
            self.got = (cands, kw)
            return "scored"

    m = Model()
    seq = torch.tensor([[5, 6, 3, 0], [5, 3, 0, 0], [7, 8, 9, 4], [0, 0, 0, 0]])         # 2 clips x 2 hypotheses, padded with 0
    assert scoring.rescore(m, dict(sequences=seq), torch.zeros(2, 4, 8), None, input_ids="ids") == "scored"
    assert m.got == ([[[5, 6, 3], [5, 3]], [[7, 8, 9, 4], [0]]], dict(append_eos=False, input_ids="ids"))
    scoring.rescore(m, seq, torch.zeros(2, 4, 8), None, eos_token_id=9)
    assert m.got[0] == [[[5, 6, 3, 0], [5, 3, 0, 0]], [[7, 8, 9], [0, 0, 0, 0]]]
    with pytest.raises(ValueError):
        scoring.rescore(m, seq[:3], torch.zeros(2, 4, 8), None)


# ============================================================================ the Python plumbing, launches stubbed out
def test_score_plumbing_under_dry_run():
    """``ASRModel.score`` end to end with the kernel launches stubbed (``_lib.DRY_RUN``: arguments are marshalled through the real
    prototypes, nothing is computed): one prompt pass per call, one ``ta_lm_score`` per chunk, with and without adapters."""
    from oracle import weights as OW
    from tiny_audio_amd import _lib
    from tiny_audio_amd.asr_config import ASRConfig
    from tiny_audio_amd.asr_modeling import ASRModel, ScoreOutput
    _lib.DRY_RUN = True
    try:
        dry = _lib.lib()
        enc, lm = OW.enc_config(hidden=256, ffn=512, layers=1, heads=4), OW.lm_config(vocab=1000, hidden=256, ffn=512, layers=2, heads=4, kv_heads=2)
        for lora in (False, True):
            cfg = ASRConfig(audio_config=enc, text_config=lm, projector_hidden_dim=128, audio_token_id=999, pad_token_id=990,
                            eos_token_id=991, use_lora=lora)
            m = ASRModel(cfg, device="cpu", init="random")
            ids = torch.tensor([[5, 6] + [999] * 12 + [7, 8]] * 2)
            kw = dict(input_ids=ids, attention_mask=torch.ones_like(ids))
            feats, amask = torch.zeros(2, 128, 100), torch.ones(2, 100, dtype=torch.int64)
            dry.calls.clear()
            out = m.score(feats, amask, [[[1, 2, 3], [4]], [[5, 6]]], return_token_scores=True, **kw)
            assert isinstance(out, ScoreOutput) and out.scores.shape == (3,) and out.token_logprobs.shape == (3, 4)
            assert out.token_ids.tolist() == [[1, 2, 3, 991], [4, 991, 0, 0], [5, 6, 991, 0]] and out.n_tokens.tolist() == [4, 2, 3]
            assert dry.calls.count("ta_lm_prefill") == 1 and dry.calls.count("ta_lm_score") == 1 and "ta_lm_decode_step" not in dry.calls
            dry.calls.clear()
            tab = scoring.build_candidate_table([[[1]] * 3, [[2, 3]] * 2], None, 991, False, max_rows=2)
            args = m._prepare_generation(ids, feats, amask, kw["attention_mask"], None, {})
            m.language_model.score_candidates(args["input_ids"], args["src_row"], args["audio"], args["attention_mask"], tab["token_ids"],
                                              tab["n_tokens"], tab["candidate_clip"], tab["chunks"])
            assert dry.calls.count("ta_lm_prefill") == 1 and dry.calls.count("ta_lm_score") == 3
            dry.calls.clear()
            assert m.score(feats, amask, [[], []], **kw).scores.shape == (0,) and "ta_lm_prefill" not in dry.calls
            with pytest.raises(ValueError, match="candidate lists for 2 clips"):
                m.score(feats, amask, [[[1]]], **kw)
            with pytest.raises(ValueError, match="outside the vocabulary"):
                m.score(feats, amask, [[[1000]], []], **kw)
    finally:
        _lib.DRY_RUN = False
        _lib._LIB = None


# ============================================================================ the C ABI's refusals
P = C.c_void_p(4096)           # a non-NULL "device pointer": a refused call never reads it


def _lm_weights(**over):
    from tiny_audio_amd import _lib
    f = dict(vocab=1024, vocab_pad=1024, hidden=256, ffn=512, n_layers=2, heads=4, kv_heads=2, head_dim=128, max_pos=512, eps=1e-6)
    f.update(over)
    return _lib.LmWeights(**f)


def test_attention_extend_refusals():
    from tiny_audio_amd import _lib
    L = _lib.lib()
    good = dict(Q=P, Kn=P, Vn=P, Kc=P, Vc=P, pmask=P, clip_of=P, len=P, O=P, LSE=None, B=2, R=3, Hq=4, Hkv=2, T=16, Lp=32, Lmax=32)
    order = ("Q", "Kn", "Vn", "Kc", "Vc", "pmask", "clip_of", "len", "O", "LSE", "B", "R", "Hq", "Hkv", "T", "Lp", "Lmax")

    def call(**over):
        a = dict(good, **over)
        return L.ta_attention_extend(*[a[k] for k in order], 0.088, None)

    for k in ("Q", "Kn", "Vn", "Kc", "Vc", "pmask", "clip_of", "len", "O"):
        assert call(**{k: None}) == 1, k
    for over in (dict(T=0), dict(T=257), dict(R=0), dict(R=1025), dict(B=0), dict(Lp=0), dict(Lp=33), dict(Hq=6, Hkv=4), dict(Hq=16, Hkv=2),
                 dict(Hq=3, Hkv=1), dict(Hkv=0), dict(Hq=0)):
        assert call(**over) == 1, over


def test_lm_score_refusals_and_workspace():
    from tiny_audio_amd import _lib
    L = _lib.lib()
    w = _lm_weights()
    B, R, T, Lp = 2, 3, 8, 40
    need = L.ta_lm_score_workspace_bytes(C.byref(w), B, R, T)
    assert need > 0
    lens = (C.c_int * R)(1, 8, 3)
    good = dict(w=C.byref(w), ids=P, len=P, len_host=lens, clip_of=P, pos0=P, B=B, R=R, T=T, kcache=P, vcache=P, Lp=Lp, pmask=P, logits=P,
                lora_img=None, token_logprobs=P, score=P, ws=P, ws_bytes=need)
    order = ("w", "ids", "len", "len_host", "clip_of", "pos0", "B", "R", "T", "kcache", "vcache", "Lp", "pmask", "logits", "lora_img",
             "token_logprobs", "score", "ws", "ws_bytes")

    def call(**over):
        a = dict(good, **over)
        return L.ta_lm_score(*[a[k] for k in order], None)

    for k in ("w", "ids", "len", "len_host", "clip_of", "pos0", "kcache", "vcache", "pmask", "logits", "token_logprobs", "score", "ws"):
        assert call(**{k: None}) == 1, k
    for over in (dict(T=0), dict(T=257), dict(R=0), dict(R=1025), dict(R=1024, T=128), dict(B=0), dict(Lp=0), dict(Lp=512 - T + 1),
                 dict(ws_bytes=need - 1), dict(len_host=(C.c_int * R)(1, 9, 3)), dict(len_host=(C.c_int * R)(0, 8, 3))):
        assert call(**over) == 1, {k: v for k, v in over.items() if k != "len_host"} or "len_host outside [1, T]"
    for bad in (dict(head_dim=64), dict(hidden=200), dict(vocab=2048), dict(heads=16, kv_heads=2), dict(heads=5, kv_heads=2), dict(n_layers=65),
                dict(lora_rank=8)):                                         # the last: adapters without their images
        wb = _lm_weights(**bad)
        assert call(w=C.byref(wb), ws_bytes=1 << 40) == 1, bad
    # the workspace query: -1 outside the limits, monotone in R and in T inside them
    for r, t in ((0, 8), (1025, 8), (3, 0), (3, 257), (1024, 128)):
        assert L.ta_lm_score_workspace_bytes(C.byref(w), B, r, t) == -1, (r, t)
    sizes_r = [L.ta_lm_score_workspace_bytes(C.byref(w), B, r, 16) for r in (1, 2, 3, 17, 64, 255, 256, 1024)]
    sizes_t = [L.ta_lm_score_workspace_bytes(C.byref(w), B, 16, t) for t in (1, 2, 15, 16, 17, 33, 64, 255, 256)]
    assert all(a > 0 for a in sizes_r + sizes_t)
    assert sizes_r == sorted(sizes_r) and sizes_t == sorted(sizes_t)

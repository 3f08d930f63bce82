"""-m gpu: candidate scoring end to end -- ``ASRModel.score`` / ``Qwen3MI355X.score_candidates`` / ``ta_lm_score`` on the
generate_small.npz model (vocab 1024, 2 layers, 4 / 2 heads), the LoRA fixture model and a SmolLM3-style tower.

Gate against the oracle (tests/score_ref.py, fp32 model + float64 log-softmax): the difference is bf16 model arithmetic against fp32 and
cannot be derived; it was measured on the first GPU run (REC below, profiles/candidate_scoring.md) and is gated at 3 x the recorded value,
the precedent of tests/test_gpu_scores.py; the recorded value must itself stay below the 0.12 the project accepts between the cache path
and the full forward.  Against ``generate`` (triangle inequality through the oracle, with the decode gate tests/test_gpu_scores.py
records): |score's lp_t - decode's lp_t| <= 3 REC + 3 * 0.02702.  Against ``generate_beams(length_penalty=0.0).sequences_scores``: the
same per token, summed, with the beam path's own recorded oracle gap per token (REC_BEAM, measured in the same run and written beside REC).
Probability identities: given one logits row each log-probability is within 5e-6 (1 + |lp|) (the softmax kernel gate) and |lp| stays
below about 20 here, so sums of 1024 probabilities are within 2e-4 of their value.  Invariances (candidate order, duplicates, ids behind
a candidate's end) are exact, bit for bit.  None of this can pass without the feature: every test calls it.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import qwen3 as OQ
from oracle import weights as OW
from tests import score_ref as SR
from tests.golden import recipe as RC

DEV = "cuda"
REC = 0.02999           # max |token_logprobs - oracle| over the oracle case below, as recorded in profiles/candidate_scoring.md
REC_BEAM = 0.00885      # max over hypotheses of |sequences_scores - oracle score| / tokens, generate_beams(num_beams=4, length_penalty=0), same file
REC_DECODE = 0.02702    # tests/test_gpu_scores.py REC_LOGPROB (profiles/decode_scores.md)
GATE = 3.0
LENS = (1, 2, 17, 40)


class _Tok:
    """Words -> ids (the fixture vocabulary has no text of its own); unknown words are dropped."""
    WORDS = {"yes": 11, "no": 12, "maybe": 13, "the": 14, "cat": 15, "sat": 16}

    def __len__(self):
        return 1024

    def __call__(self, text, add_special_tokens=True):
        assert add_special_tokens is False
        return {"input_ids": [self.WORDS[w] for w in text.split() if w in self.WORDS]}


class _Ctx:
    pass


@pytest.fixture(scope="module")
def ctx(golden):
    from tests.test_gpu_parity import build_model
    g = golden("generate_small.npz")
    S = RC.SMALL
    E, D, H = S["enc"]["hidden"], S["lm"]["hidden"], S["proj_hidden"]
    wE, wL, wP = OW.init_encoder(S["enc"], 0), RC.gen_lm_weights(), OW.init_mlp_projector(E, D, H)
    c = _Ctx()
    c.m = build_model(S["enc"], S["lm"], H, wE, wL, wP, audio_token_id=S["audio_token_id"], pad_token_id=S["pad_id"], eos_token_id=S["eos_id"])
    c.m.tokenizer = _Tok()
    c.feats, c.amask = torch.from_numpy(g["input_features"]), torch.from_numpy(g["audio_attention_mask"])
    c.prompt = dict(input_ids=torch.from_numpy(g["input_ids"]), attention_mask=torch.ones(g["input_ids"].shape, dtype=torch.int64))
    c.W = dict(encoder=wE, lm=wL, projector=wP)
    c.cfg = dict(enc=S["enc"], lm=S["lm"], projector_type="mlp", k=S["k"], audio_token_id=S["audio_token_id"])
    c.x = SR.prompt_rows(dict(input_ids=g["input_ids"], input_features=g["input_features"]), c.W, c.cfg)      # computed once, shared
    c.V, c.eos, c.pad = S["lm"]["vocab"], S["eos_id"], S["pad_id"]
    rng = np.random.RandomState(5)
    c.cands = [[rng.randint(0, 1000, n).tolist() for n in LENS] for _ in range(2)]
    c.ref = SR.token_logprobs(c.x, c.W, c.cfg, c.cands)
    return c


def _score(ctx, cands, **kw):
    return ctx.m.score(ctx.feats, ctx.amask, cands, **ctx.prompt, **kw)


def _gap(out, ref):
    """max |token_logprobs - reference| over the candidates' own tokens; also checks the exact zeros behind each end."""
    lp, n = out.token_logprobs.cpu().numpy(), out.n_tokens.tolist()
    flat = [r for clip in ref for r in clip]
    worst = 0.0
    for r, want in enumerate(flat):
        assert n[r] == len(want) and not lp[r, n[r]:].any(), "token_logprobs must be exact 0 behind a candidate's end"
        worst = max(worst, float(np.abs(lp[r, :n[r]] - want).max()))
    return worst


@pytest.mark.parametrize("residual", ("bfloat16", "float32"))
def test_token_logprobs_against_the_oracle(ctx, residual):
    ctx.m.config.residual_dtype = residual
    try:
        out = _score(ctx, ctx.cands, append_eos=False, return_token_scores=True)
    finally:
        ctx.m.config.residual_dtype = None
    assert out.scores.shape == (8,) and out.token_logprobs.shape == (8, 40) and out.candidate_clip.tolist() == [0] * 4 + [1] * 4
    assert torch.equal(out.token_ids, torch.tensor([c + [0] * (40 - len(c)) for clip in ctx.cands for c in clip]))
    d = _gap(out, ctx.ref)
    print(f"score vs oracle ({residual} residual stream): max |token_logprobs - oracle| = {d:.5f} over {sum(LENS) * 2} tokens")
    lp = out.token_logprobs.cpu().numpy()
    want = np.zeros(8, np.float32)
    for t in range(lp.shape[1]):                            # the row sum in index order, f32
        want = (want + lp[:, t]).astype(np.float32)
    assert np.array_equal(out.scores.cpu().numpy(), want)
    assert (lp <= 0).all() and np.isfinite(lp).all()
    assert REC <= 0.12
    assert d <= GATE * REC


def test_against_generate_token_scores(ctx):
    """The greedy tokens of generate(return_token_scores=True), no processors: scoring them gives the decode step's log-probabilities."""
    o = ctx.m.generate(input_features=ctx.feats, audio_attention_mask=ctx.amask, **ctx.prompt, max_new_tokens=12, eos_token_id=[],
                       return_token_scores=True)
    seq, dec = o.sequences.cpu(), o.token_logprobs.cpu().numpy()
    out = _score(ctx, [[seq[0].tolist()], [seq[1].tolist()]], append_eos=False, return_token_scores=True)
    d = float(np.abs(out.token_logprobs.cpu().numpy() - dec).max())
    print(f"score vs generate: max |lp_t - decode's lp_t| = {d:.5f} over {seq.numel()} tokens")
    assert d <= GATE * REC + GATE * REC_DECODE


def test_against_beam_sequences_scores(ctx):
    from tiny_audio_amd import scoring
    kw = dict(input_features=ctx.feats, audio_attention_mask=ctx.amask, **ctx.prompt)
    o = ctx.m.generate_beams(**kw, num_beams=4, length_penalty=0.0, num_return_sequences=4, max_new_tokens=10, eos_token_id=[ctx.eos, ctx.pad])
    out = scoring.rescore(ctx.m, o, ctx.feats, ctx.amask, **ctx.prompt)
    n = out.n_tokens.numpy()
    cands = [[row[:k] for row, k in zip(o.sequences.cpu()[b * 4:(b + 1) * 4].tolist(), n[b * 4:(b + 1) * 4])] for b in range(2)]
    ref = np.array([s for clip in SR.scores(ctx.x, ctx.W, ctx.cfg, cands) for s in clip])
    beam, mine = o.sequences_scores.cpu().numpy().astype(np.float64), out.scores.cpu().numpy().astype(np.float64)
    g_beam, g_mine, g = np.abs(beam - ref) / n, np.abs(mine - ref) / n, np.abs(mine - beam) / n
    print(f"beams: per token, max |sequences_scores - oracle| = {g_beam.max():.5f}, |rescore - oracle| = {g_mine.max():.5f}, "
          f"|rescore - sequences_scores| = {g.max():.5f}; lengths {n.tolist()}")
    assert out.candidate_clip.tolist() == [0] * 4 + [1] * 4 and (n >= 1).all()
    assert g_beam.max() <= GATE * REC_BEAM and g_mine.max() <= GATE * REC
    assert (np.abs(mine - beam) <= n * (GATE * REC + GATE * REC_BEAM)).all()


def test_probability_identities(ctx):
    V = ctx.V
    one = _score(ctx, [[[v] for v in range(V)], []], append_eos=False)
    total = float(np.exp(one.scores.cpu().numpy().astype(np.float64)).sum())
    c0 = ctx.cands[1][0][0]
    base = float(_score(ctx, [[], [[c0]]], append_eos=False).scores[0])
    two = _score(ctx, [[], [[c0, v] for v in range(V)]], append_eos=False)
    marg = float(np.exp(two.scores.cpu().numpy().astype(np.float64)).sum())
    print(f"sum over 1024 one-token candidates of exp(score) - 1 = {total - 1:.2e}; two-token marginal / exp(score(c_0)) - 1 = "
          f"{marg / np.exp(base) - 1:.2e}; min score {float(two.scores.min()):.2f}")
    assert one.scores.shape == (V,) and two.n_tokens.tolist() == [2] * V
    assert abs(total - 1.0) <= 2e-4
    assert abs(marg - np.exp(base)) <= 2e-4 * np.exp(base)


def test_exact_invariances(ctx):
    base = _score(ctx, ctx.cands, append_eos=False, return_token_scores=True)
    # the candidates of a call permuted (within and across the clips' lists), and one of them given twice
    perm = [[ctx.cands[0][i] for i in (2, 0, 3, 1)] + [ctx.cands[0][2]], [ctx.cands[1][i] for i in (3, 2, 1, 0)]]
    back = [1, 3, 0, 2, 8, 7, 6, 5]                       # row of `p` that holds candidate r of `base`
    p = _score(ctx, perm, append_eos=False, return_token_scores=True)
    assert torch.equal(p.scores[back].cpu(), base.scores.cpu()) and torch.equal(p.token_logprobs[back].cpu(), base.token_logprobs.cpu())
    assert torch.equal(p.scores[4].cpu(), p.scores[0].cpu()) and torch.equal(p.token_logprobs[4].cpu(), p.token_logprobs[0].cpu())
    # different garbage ids behind each candidate's end
    ctx.m.eval()
    args = ctx.m._prepare_generation(ctx.prompt["input_ids"], ctx.feats, ctx.amask, ctx.prompt["attention_mask"], None, {})
    lm, pa = ctx.m.language_model, (args["input_ids"], args["src_row"], args["audio"], args["attention_mask"])
    ids, n, clip = base.token_ids.clone(), base.n_tokens, base.candidate_clip
    behind = torch.arange(ids.shape[1])[None, :] >= n[:, None]
    lp0, s0 = lm.score_candidates(*pa, ids, n, clip)
    ids[behind] = torch.randint(0, 1 << 40, ids.shape)[behind] - (1 << 39)             # in and far outside the vocabulary, both signs
    lp1, s1 = lm.score_candidates(*pa, ids, n, clip)
    assert torch.equal(lp0, lp1) and torch.equal(s0, s1)
    assert torch.equal(s0.cpu(), base.scores.cpu()) and torch.equal(lp0.cpu(), base.token_logprobs.cpu())


def test_strings_eos_empty_clip_and_refusals(ctx):
    a = _score(ctx, [["yes no", [7, 8, 9]], []], return_token_scores=True)               # append_eos defaults to True
    b = _score(ctx, [[[11, 12, ctx.eos], [7, 8, 9, ctx.eos]], []], append_eos=False, return_token_scores=True)
    assert a.n_tokens.tolist() == [3, 4] and a.candidate_clip.tolist() == [0, 0] and torch.equal(a.token_ids, b.token_ids)
    assert torch.equal(a.scores.cpu(), b.scores.cpu()) and torch.equal(a.token_logprobs.cpu(), b.token_logprobs.cpu())
    pc = a.per_clip()
    assert [len(c) for c in pc] == [2, 0] and pc[0][1]["token_ids"] == [7, 8, 9, ctx.eos] and len(pc[0][0]["token_logprobs"]) == 3
    none = _score(ctx, [[], []])
    assert none.scores.shape == (0,) and none.per_clip() == [[], []]
    from tiny_audio_amd import scoring
    assert scoring.pick(a.scores, a.n_tokens, a.candidate_clip, n_clips=2)[1] == -1
    for bad in ([["zebra"], []], [[[5, 1024]], []], [[[1] * 257], []], [[[1]]]):
        with pytest.raises(ValueError):
            _score(ctx, bad)
    lm_cfg = ctx.m.language_model.config
    max_pos = lm_cfg.max_position_embeddings
    lm_cfg.max_position_embeddings = ctx.prompt["input_ids"].shape[1] + 3
    try:
        assert _score(ctx, [[[1, 2, 3]], []], append_eos=False).scores.shape == (1,)
        with pytest.raises(ValueError, match="max_position_embeddings"):
            _score(ctx, [[[1, 2, 3]], []])                   # the appended eos is the fourth token
    finally:
        lm_cfg.max_position_embeddings = max_pos


# ============================================================================ LM level: adapters, a SmolLM3-style tower, padded prompts
def _lm_score(lm, x, att, cands):
    from tiny_audio_amd import scoring
    B, L, D = x.shape
    ids = torch.full((B, L), lm.config.vocab_size - 1, dtype=torch.int64, device=DEV)
    src = torch.arange(B * L, dtype=torch.int32, device=DEV)
    tab = scoring.build_candidate_table(cands, None, 0, False, vocab_size=lm.config.vocab_size)
    lp, sc = lm.score_candidates(ids, src, torch.from_numpy(x.reshape(B * L, D)).to(DEV), torch.from_numpy(att).to(DEV), tab["token_ids"],
                                 tab["n_tokens"], tab["candidate_clip"])
    return tab, lp.cpu().numpy(), sc.cpu().numpy()


def _lm_gap(x, att, embed, cands, lp, forward, V):
    """max |lp - reference| with the reference's logits from ``forward`` (inputs_embeds [K, Lv + T, D] of one clip's valid prompt rows
    followed by the candidates -> logits), float64 log-softmax."""
    worst, r = 0.0, 0
    for b, mine in enumerate(cands):
        xv = x[b][att[b].astype(bool)]
        T = max(len(c) for c in mine)
        ids = np.zeros((len(mine), T), np.int64)
        for k, c in enumerate(mine):
            ids[k, :len(c)] = c
        logits = forward(np.concatenate([np.repeat(xv[None], len(mine), 0), embed[ids]], axis=1).astype(np.float32))
        lsm = SR.log_softmax64(logits[:, len(xv) - 1:len(xv) - 1 + T, :V])
        for k, c in enumerate(mine):
            want = lsm[k, np.arange(len(c)), np.asarray(c)]
            assert not lp[r, len(c):].any()
            worst = max(worst, float(np.abs(lp[r, :len(c)] - want).max()))
            r += 1
    return worst


def test_lora_model_against_the_oracle():
    """The lora_small.npz model (r = 8, alpha 32, all seven linears) on its inputs_embeds fixture; clip 1 is right-padded, so its
    masked cache slots lie between the prompt and the candidates."""
    from tiny_audio_amd.language_model import LMConfig, Qwen3MI355X
    cfg = RC.SMALL["lm"]
    wL, lo = OW.init_lm(cfg, seed=1), OW.init_lora(cfg, rank=8, seed=4)
    lm = Qwen3MI355X(LMConfig(cfg), DEV).load_state_dict_hf(wL)
    lm.enable_lora(rank=8, alpha=32).load_lora_state_dict(lo)
    x, att, _ = RC.lm_input()
    rng = np.random.RandomState(9)
    cands = [[rng.randint(0, 1000, n).tolist() for n in (1, 17)], [rng.randint(0, 1000, n).tolist() for n in (2, 40)]]
    _, lp, _ = _lm_score(lm, x, att, cands)
    embed = wL["model.embed_tokens.weight"]
    fwd = lambda lora: (lambda xc: OQ.lm_forward(xc, np.ones(xc.shape[:2], np.int64), wL, cfg, keep_cache=False, lora=lora,  # noqa: E731
                                                 lora_scale=4.0 if lora else 0.0)[0])
    d, d_base = _lm_gap(x, att, embed, cands, lp, fwd(lo), cfg["vocab"]), _lm_gap(x, att, embed, cands, lp, fwd(None), cfg["vocab"])
    print(f"LoRA model: max |token_logprobs - oracle| = {d:.5f} (against the oracle WITHOUT adapters: {d_base:.3f})")
    assert d <= GATE * REC
    assert d_base > 10 * GATE * REC, "the adapters must matter in this case, otherwise it proves nothing about them"


def test_smollm3_style_tower_against_transformers():
    """No q/k-norm, the second of two layers NoPE, 4 query heads on 1 kv head; clip 0 right-padded, clip 1 left-padded."""
    from tests.test_gpu_smollm3 import hip_lm, ragged_batch, tower
    model, w, src = tower("smollm3", 4, 1, layers=2, no_rope_layers=[1, 0])
    lm = hip_lm(w, src)
    assert lm._w.nope_layers == 0b10 and lm._layers_arr[0].qn_w is None
    x, att, _, _ = ragged_batch(2, 40)
    rng = np.random.RandomState(3)
    V = lm.config.vocab_size
    cands = [[rng.randint(0, V - 1, n).tolist() for n in (1, 2, 17)], [rng.randint(0, V - 1, n).tolist() for n in (40,)]]
    _, lp, _ = _lm_score(lm, x, att, cands)

    def fwd(xc):
        with torch.no_grad():
            return model(inputs_embeds=torch.from_numpy(xc), use_cache=False).logits.float().numpy()
    d = _lm_gap(x, att, w["model.embed_tokens.weight"], cands, lp, fwd, V)
    print(f"SmolLM3-style tower: max |token_logprobs - transformers fp32| = {d:.5f}")
    assert d <= GATE * REC

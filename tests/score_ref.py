"""Reference for candidate scoring (``ASRModel.score`` / ``ta_lm_score``).  TEST INFRASTRUCTURE ONLY.

For clip b with prompt P_b and candidate c = (c_0 .. c_{n-1}):  lp_t = log_softmax(z(P_b, c_<t))[c_t], score = sum_t lp_t.  The logits
are the fp32 oracle's (``oracle.qwen3.lm_forward`` over prompt + candidate, one causal pass: position L - 1 + t predicts c_t, and the
padding behind a shorter candidate cannot reach the positions before it); the log-softmax and the sum are float64.  The prompt is the
batch's ``input_ids`` with every position valid, as in the fixtures.  ``tests/test_score_ref.py`` pins this against
``tests/scores_ref.teacher_forced_logits`` (the step-by-step restatement of greedy decoding) and against the identities of a
probability distribution.
"""
import numpy as np

from oracle import generate as OG
from oracle import qwen3 as OQ


def log_softmax64(z):
    z = np.asarray(z, np.float64)
    m = z.max(-1, keepdims=True)
    return z - m - np.log(np.exp(z - m).sum(-1, keepdims=True))


def prompt_rows(batch, W, cfg):
    """inputs_embeds of the prompts [B, L, D] (audio rows in place): compute once, share among the tests of a module."""
    return OG.prompt_embeds(batch, W, cfg)


def token_logprobs(x_prompt, W, cfg, candidates):
    """x_prompt [B, L, D] from ``prompt_rows``; ``candidates``: one list of token-id lists per clip -> one list per clip of float64
    arrays lp [n] (an empty list for a clip without candidates)."""
    embed = W["lm"]["model.embed_tokens.weight"]
    V = cfg["lm"]["vocab"]
    out = []
    for b, cands in enumerate(candidates):
        if not cands:
            out.append([])
            continue
        L, T = x_prompt.shape[1], max(len(c) for c in cands)
        ids = np.zeros((len(cands), T), np.int64)
        for k, c in enumerate(cands):
            ids[k, :len(c)] = c
        x = np.concatenate([np.repeat(x_prompt[b:b + 1], len(cands), 0), embed[ids]], axis=1)
        logits, _ = OQ.lm_forward(x, np.ones(x.shape[:2], np.int64), W["lm"], cfg["lm"], keep_cache=False, lora=W.get("lora"),
                                  lora_scale=cfg.get("lora_scale", 0.0))
        lsm = log_softmax64(logits[:, L - 1:L - 1 + T, :V])
        out.append([lsm[k, np.arange(len(c)), np.asarray(c, np.int64)] for k, c in enumerate(cands)])
    return out


def scores(x_prompt, W, cfg, candidates):
    """-> one list per clip of float64 scores (the sum of ``token_logprobs`` in the order t = 0 .. n-1)."""
    return [[float(np.sum(lp)) for lp in clip] for clip in token_logprobs(x_prompt, W, cfg, candidates)]

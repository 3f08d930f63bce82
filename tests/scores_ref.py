"""References for the decoding scores (``ta_token_scores_f32``).  TEST INFRASTRUCTURE ONLY.

``token_scores_ref``: fp64 numpy restatement of the kernel's contract (include/ta355.h) -- log-probability of the chosen token, entropy
and the top-k alternatives of one step's logits, with the same tie rule (lowest index first) and the same -inf rules (a -inf entry has
probability 0 and contributes 0 to the entropy; a chosen -inf gives -inf; slots beyond the finite entries are (-1, -inf)).
``tests/test_scores_ref.py`` checks it against closed forms and ``torch.log_softmax`` in float64.

``teacher_forced_logits``: the loop of ``oracle.generate.greedy_generate`` (imported, not modified) restated with the tokens GIVEN
instead of chosen, returning every step's processed f32 logits -- the rows the device scores.
"""
import numpy as np

from oracle import generate as OG
from oracle import qwen3 as OQ


def token_scores_ref(x, V, chosen, top_k):
    """x [B, ld] (columns >= V ignored), chosen int [B] -> (logprob f64 [B], entropy f64 [B], top_ids i64 [B, top_k],
    top_logprobs f64 [B, top_k])."""
    x = np.asarray(x)[:, :V].astype(np.float64)
    B = x.shape[0]
    logprob, entropy = np.zeros(B), np.zeros(B)
    top_ids, top_lp = np.full((B, top_k), -1, np.int64), np.full((B, top_k), -np.inf)
    for b in range(B):
        row = x[b]
        fin = np.isfinite(row)
        if not fin.any():                                   # nothing has any probability
            logprob[b] = -np.inf
            continue
        m = row[fin].max()
        e = np.where(fin, np.exp(np.where(fin, row - m, 0.0)), 0.0)
        lz = m + np.log(e.sum())
        lp = np.where(fin, np.where(fin, row, 0.0) - lz, -np.inf)
        p = np.exp(lp)
        logprob[b] = lp[int(chosen[b])]
        entropy[b] = -float(np.sum(np.where(p > 0, p * np.where(p > 0, lp, 0.0), 0.0)))
        order = np.lexsort((np.arange(V), -row))            # descending value, ascending index on ties
        order = order[fin[order]][:top_k]
        top_ids[b, :order.size] = order
        top_lp[b, :order.size] = lp[order]
    return logprob, entropy, top_ids, top_lp


def teacher_forced_logits(batch, W, cfg, tokens, eos_ids=(), repetition_penalty=1.0, no_repeat_ngram_size=0, processors_see_prompt=True,
                          min_new_tokens=0):
    """-> (list over steps of processed logits f32 [B, V], unfinished bool [B, n_new]: True where the clip had not finished BEFORE the
    step).  Step t sees the prompt and ``tokens[:, :t]``; the logits processors and the eos suppression are applied exactly as
    ``oracle.generate.greedy_generate`` applies them (same functions, same order)."""
    tokens = np.asarray(tokens, np.int64)
    B, n_new = tokens.shape
    x = OG.prompt_embeds(batch, W, cfg)
    embed = W["lm"]["model.embed_tokens.weight"]
    unfinished = np.ones(B, dtype=bool)
    steps, alive = [], np.zeros((B, n_new), dtype=bool)
    for t in range(n_new):
        logits, _ = OQ.lm_forward(x, np.ones(x.shape[:2], np.int64), W["lm"], cfg["lm"], keep_cache=False,
                                  lora=W.get("lora"), lora_scale=cfg.get("lora_scale", 0.0))
        last = logits[:, -1].astype(np.float32)
        if repetition_penalty != 1.0 or no_repeat_ngram_size > 0:
            head = [np.asarray(batch["input_ids"], np.int64)] if processors_see_prompt else [np.zeros((B, 0), np.int64)]
            seq = np.concatenate(head + [tokens[:, :t]], axis=1)
            last = OG.apply_logits_processors(last, seq, repetition_penalty, no_repeat_ngram_size)
        if t < min_new_tokens and len(eos_ids):
            last = last.copy()
            last[:, np.asarray(list(eos_ids), dtype=np.int64)] = -np.inf
        steps.append(last)
        alive[:, t] = unfinished
        unfinished = unfinished & ~np.isin(tokens[:, t], np.asarray(list(eos_ids), dtype=np.int64))
        x = np.concatenate([x, embed[tokens[:, t]][:, None, :]], axis=1)
    return steps, alive

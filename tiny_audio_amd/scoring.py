"""Candidate scoring: the log-probability of GIVEN texts under the model (``ASRModel.score``), host side.

For clip b with prompt P_b and a candidate c = (c_0 .. c_{n-1}):  lp_t = log_softmax(z(P_b, c_<t))[c_t],  score = sum_t lp_t -- minus
HF's summed cross-entropy of those label positions (the ``labels`` path of tiny_audio/asr_modeling.py:481-533), computed with the clip's
prompt cache shared by its candidates (include/ta355.h ``ta_lm_score``).  This module is the packing and the uses built on the scores:

* ``build_candidate_table``: ragged per-clip candidate lists (strings and / or token-id lists) -> one padded id table, pure host code;
* ``pick``: the winning candidate per clip (closed-set tasks: what scripts/eval/evaluators/mcq.py:89-132 and classification.py get by
  generating free text and string-matching the choices);
* ``rescore``: the hypotheses of a ``generate_beams`` result scored again, e.g. under another prompt or adapter, or to verify
  ``sequences_scores`` from outside the beam kernels.
"""
from __future__ import annotations

import re

import torch

from . import _lib


def limits():
    """(max rows, max tokens per row, max rows * tokens) of one ``ta_lm_score`` call, read from include/ta355.h."""
    text = open(_lib.HEADER).read()
    get = lambda name: int(re.search(rf"#define {name} (\d+)", text).group(1))  # noqa: E731
    return get("TA_EXTEND_MAX_R"), get("TA_EXTEND_MAX_T"), get("TA_SCORE_MAX_ROWS")


def chunk_rows(n_tokens, max_rows, max_tokens, max_cells):
    """Consecutive row ranges [(r0, r1)] such that every range has at most ``max_rows`` rows and rows * (its longest row) <=
    ``max_cells``: the calls ``Qwen3MI355X.score_candidates`` makes.  A row longer than ``max_tokens`` is a ValueError."""
    n = [int(v) for v in n_tokens]
    if any(v > max_tokens for v in n):
        raise ValueError(f"a candidate has {max(n)} tokens; one scoring call takes at most {max_tokens}")
    out, r0, longest = [], 0, 0
    for r, v in enumerate(n):
        grown = max(longest, v)
        if r > r0 and (r - r0 + 1 > max_rows or (r - r0 + 1) * grown > max_cells):
            out.append((r0, r))
            r0, grown = r, v
        longest = grown
    if len(n) > r0:
        out.append((r0, len(n)))
    return out


def build_candidate_table(candidates, tokenizer, eos_id, append_eos, vocab_size=None, max_rows=None, max_cells=None):
    """``candidates``: one list per clip; an entry is a ``str`` (tokenised with ``add_special_tokens=False``) or a list of token ids.
    The lists are ragged and a clip may have none.  ``append_eos`` appends ``eos_id`` (what training labels end with) to every
    candidate.  -> dict(token_ids int64 [R, T] padded with 0, n_tokens int64 [R], candidate_clip int64 [R], n_clips, chunks), rows
    clip-major in the given order, T the longest candidate, ``chunks`` the row ranges of ``chunk_rows`` under the C limits (or the given
    ``max_rows`` / ``max_cells``).  ValueError: a candidate that is empty after tokenisation, an id outside [0, vocab_size)
    (``vocab_size`` None: ``len(tokenizer)`` when a tokenizer is given, else unchecked)."""
    if vocab_size is None and tokenizer is not None:
        vocab_size = len(tokenizer)
    lim_r, lim_t, lim_c = limits()
    max_rows = lim_r if max_rows is None else int(max_rows)
    max_cells = lim_c if max_cells is None else int(max_cells)
    rows, clip = [], []
    for b, cands in enumerate(candidates):
        for j, c in enumerate(cands):
            if isinstance(c, str):
                if tokenizer is None:
                    raise ValueError(f"clip {b} candidate {j} is a string and no tokenizer is attached")
                ids = tokenizer(c, add_special_tokens=False)["input_ids"]
            else:
                ids = c.tolist() if torch.is_tensor(c) else list(c)
            ids = [int(t) for t in ids]
            if not ids:
                raise ValueError(f"clip {b} candidate {j} is empty after tokenisation")
            if append_eos:
                ids.append(int(eos_id))
            bad = [t for t in ids if t < 0 or (vocab_size is not None and t >= vocab_size)]
            if bad:
                raise ValueError(f"clip {b} candidate {j}: token id {bad[0]} is outside the vocabulary [0, {vocab_size})")
            rows.append(ids)
            clip.append(b)
    R, T = len(rows), max((len(r) for r in rows), default=0)
    table = torch.zeros((R, T), dtype=torch.int64)
    for r, ids in enumerate(rows):
        table[r, :len(ids)] = torch.tensor(ids, dtype=torch.int64)
    n_tokens = torch.tensor([len(r) for r in rows], dtype=torch.int64)
    return dict(token_ids=table, n_tokens=n_tokens, candidate_clip=torch.tensor(clip, dtype=torch.int64), n_clips=len(candidates),
                chunks=chunk_rows(n_tokens.tolist(), max_rows, lim_t, max_cells))


def pick(scores, n_tokens, candidate_clip, normalize="sum", n_clips=None):
    """The winning candidate of every clip: its index within the clip's own list (-1 for a clip without candidates), lowest index on
    ties.  ``normalize``: "sum" compares the scores, "mean" the scores divided by the token counts (length-normalised)."""
    if normalize not in ("sum", "mean"):
        raise ValueError(f"normalize must be 'sum' or 'mean'; got {normalize!r}")
    s = torch.as_tensor(scores).detach().to("cpu", torch.float64)
    n = torch.as_tensor(n_tokens).to("cpu", torch.float64)
    clip = [int(c) for c in torch.as_tensor(candidate_clip).tolist()]
    if normalize == "mean":
        s = s / n
    B = (max(clip) + 1 if clip else 0) if n_clips is None else int(n_clips)
    best, best_v, seen = [-1] * B, [None] * B, [0] * B
    for v, b in zip(s.tolist(), clip):
        if best_v[b] is None or v > best_v[b]:
            best[b], best_v[b] = seen[b], v
        seen[b] += 1
    return best


def rescore(model, generation_output, input_features=None, audio_attention_mask=None, eos_token_id=None, **score_kwargs):
    """Scores the sequences of a ``generate_beams`` result again with ``model.score``: rows [B * n, n_new] are the n hypotheses of clip
    0, then of clip 1, ...; every row is cut behind its first eos id (``eos_token_id``: an id or a list; default the model's
    ``[eos_token_id, pad_token_id]``, the stopping ids of generation), which belongs to the hypothesis.  -> ``ScoreOutput``; with
    ``length_penalty=0.0`` its ``scores`` are what ``sequences_scores`` holds."""
    seq = generation_output["sequences"] if not torch.is_tensor(generation_output) else generation_output
    seq = seq.detach().cpu()
    B = int(input_features.shape[0])
    if seq.shape[0] % B:
        raise ValueError(f"{seq.shape[0]} sequences do not divide over {B} clips")
    per = seq.shape[0] // B
    eos = eos_token_id if eos_token_id is not None else [model.config.eos_token_id, model.config.pad_token_id]
    eos = {int(e) for e in (eos if isinstance(eos, (list, tuple)) else [eos]) if e is not None}
    cands = []
    for b in range(B):
        mine = []
        for row in seq[b * per:(b + 1) * per].tolist():
            cut = next((i + 1 for i, t in enumerate(row) if t in eos), len(row))
            mine.append(row[:cut])
        cands.append(mine)
    return model.score(input_features, audio_attention_mask, cands, append_eos=False, **score_kwargs)

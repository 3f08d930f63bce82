"""Word confidence from the decoding scores (host only: a few hundred tokens per clip).

``ASRModel.generate(return_token_scores=True)`` gives one log-probability per emitted token; a user reads words.  ``word_confidences``
maps tokens to the whitespace-separated words of the decoded text -- the split ``alignment._group_words`` uses, so the entries line up
with ``ForcedAligner``'s word timestamps and ``attach_confidence`` can copy the confidence onto them.
"""
from __future__ import annotations

import math
from typing import Callable, Iterable, Sequence

_INCOMPLETE = "\ufffd"      # what a byte-level tokenizer decodes an unfinished multi-byte character to


def _as_list(x, conv):
    if hasattr(x, "tolist"):
        x = x.tolist()
    return [conv(v) for v in x]


def word_confidences(token_ids, token_logprobs, eos_ids: Iterable[int], decode: Callable[[Sequence[int]], str]) -> list[dict]:
    """One clip: ``token_ids`` / ``token_logprobs`` are row b of ``GenerationOutput.sequences`` / ``.token_logprobs`` (1-D, any
    sequence or tensor), ``decode(ids) -> str`` the tokenizer's decoder (``lambda ids: tok.decode(ids, skip_special_tokens=True)``).
    -> one ``{"word", "logprob", "confidence", "min_prob", "n_tokens"}`` per word of ``decode(tokens before the first eos id).split()``.

    Prefixes are decoded incrementally and a token owns the characters its prefix adds.  A prefix that ends in an incomplete
    multi-byte character is held back: its tokens own, together with the token that completes it, the characters that appear then.
    A token belongs to every word of which it owns a non-whitespace character (a token spanning two words counts in both; a token
    that is only whitespace in none).  ``logprob`` is the sum over the word's tokens, ``confidence = exp(logprob / n_tokens)`` (the
    geometric mean of the token probabilities) and ``min_prob = exp(min token logprob)``.  The eos token and the pad behind it are
    ignored."""
    ids, lps = _as_list(token_ids, int), _as_list(token_logprobs, float)
    if len(ids) != len(lps):
        raise ValueError(f"word_confidences: {len(ids)} token ids but {len(lps)} log-probabilities")
    eos = {int(e) for e in eos_ids}
    n = next((i for i, t in enumerate(ids) if t in eos), len(ids))        # everything from the first eos id on is eos / pad
    ids, lps = ids[:n], lps[:n]
    owners: list[tuple] = []                       # per character of the text: the tokens that own it
    text, pending = "", []
    for i in range(n):
        pending.append(i)
        cur = decode(ids[: i + 1])
        if cur.endswith(_INCOMPLETE):
            continue
        if len(cur) > len(text):
            owners += [tuple(pending)] * (len(cur) - len(text))
        elif len(cur) < len(text):                 # a decoder that rewrote its earlier output (clean-up rules): keep what still stands
            owners = owners[: len(cur)]
        text, pending = cur, []
    out, k, L = [], 0, len(text)
    while k < L:
        if text[k].isspace():
            k += 1
            continue
        j = k
        while j < L and not text[j].isspace():
            j += 1
        toks = sorted({t for c in range(k, j) for t in owners[c]})
        lp = math.fsum(lps[t] for t in toks)
        out.append({"word": text[k:j], "logprob": lp, "confidence": math.exp(lp / len(toks)) if toks else 0.0,
                    "min_prob": math.exp(min(lps[t] for t in toks)) if toks else 0.0, "n_tokens": len(toks)})
        k = j
    return out


def attach_confidence(words: list[dict], confidences: list[dict]) -> list[dict]:
    """Copy ``confidence`` of ``word_confidences`` onto the word dicts of ``ForcedAligner.align`` (in place; returns ``words``).  Both
    lists must hold the same words in the same order; otherwise ValueError names the first mismatch (the aligned text is no longer
    the decoded one, e.g. after ``truncate_repetitions`` shortened it)."""
    for i, (w, c) in enumerate(zip(words, confidences)):
        if w["word"] != c["word"]:
            raise ValueError(f"attach_confidence: word {i} is {w['word']!r} in the alignment but {c['word']!r} in the confidences")
    if len(words) != len(confidences):
        i = min(len(words), len(confidences))
        have = "the alignment" if len(words) > i else "the confidences"
        extra = (words if len(words) > i else confidences)[i]["word"]
        raise ValueError(f"attach_confidence: {len(words)} aligned words but {len(confidences)} confidences: word {i} ({extra!r}) is "
                         f"only in {have}")
    for w, c in zip(words, confidences):
        w["confidence"] = c["confidence"]
    return words

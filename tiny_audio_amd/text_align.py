"""Text alignment on the device: WER / CER error counts and the LCS word matching of the reference's timestamp evaluator.

The string work (normalising, splitting, mapping strings to ids) is done here on the host; the O(n m) tables and their walks run in
``torch.ops.ta355.text_align`` (csrc/text_align.hip).  Contract: DESIGN.md section 3, "Text alignment" (tests/text_align_ref.py).

* ``encode``                     strings -> ragged int32 ids, one dictionary per call (``"char"``: the code points).
* ``error_counts``               per-pair distance, hits / substitutions / deletions / insertions and lengths, and the corpus rate
                                 sum(dist) / sum(ref_len) -- what ``jiwer.wer`` / ``jiwer.cer`` return for the reference's evaluator
                                 (scripts/eval/evaluators/base.py:114,150) and what ``eval_text.word_error_rate`` computes.
* ``align_words_to_reference``   the reference's function of that name (scripts/eval/evaluators/alignment.py:12-79): same signature,
                                 same list of (pred_word, ref_word) pairs; the ``<unk>`` and empty-after-normalisation skips on the
                                 host, the LCS table and its backtrack on the device.

Text normalisers are out of scope: the caller passes ``normalize`` / ``normalizer``.
"""
from __future__ import annotations

from typing import Callable, Optional, Sequence

import numpy as np
import torch

from . import _lib
from . import torch_ops  # noqa: F401  (registers torch.ops.ta355.text_align)
from .ops import TEXT_ALIGN_EDIT, TEXT_ALIGN_LCS, TEXT_ALIGN_LIMITS


def _ragged(seqs):
    cu = np.zeros(len(seqs) + 1, np.int64)
    if seqs:
        cu[1:] = np.cumsum([len(s) for s in seqs])
    if cu[-1] >= 2 ** 31:
        raise ValueError(f"{int(cu[-1])} symbols in one batch: the offsets are int32")
    flat = np.fromiter((x for s in seqs for x in s), np.int32, int(cu[-1]))
    return flat, cu.astype(np.int32)


def encode(refs: Sequence[str], hyps: Sequence[str], unit: str = "word", normalize: Optional[Callable[[str], str]] = None):
    """-> (ref_ids, cu_ref, hyp_ids, cu_hyp): int32 numpy arrays, pair p owning ids[cu[p]:cu[p + 1]].  ``unit="word"``: the
    whitespace-separated words of ``normalize(text)``, numbered by one dictionary for the whole call (only equality matters);
    ``unit="char"``: the code points of ``normalize(text)``."""
    if isinstance(refs, str):
        refs, hyps = [refs], [hyps]
    if len(refs) != len(hyps):
        raise ValueError("references and hypotheses differ in length")
    norm = normalize or (lambda s: s)
    if unit == "word":
        table: dict = {}
        ids = lambda text: [table.setdefault(w, len(table)) for w in norm(text).split()]      # noqa: E731
    elif unit == "char":
        ids = lambda text: [ord(c) for c in norm(text)]                                       # noqa: E731
    else:
        raise ValueError(f"unit {unit!r}: 'word' or 'char'")
    r, cu_r = _ragged([ids(t) for t in refs])
    h, cu_h = _ragged([ids(t) for t in hyps])
    return r, cu_r, h, cu_h


def _device_align(r, cu_r, h, cu_h, mode, want_path, device, col_block=0, row_block=0):
    """The numpy batch of ``encode`` through the operator, in calls of at most ``TEXT_ALIGN_LIMITS['pairs']`` pairs ->
    (dist [N], counts [N, 4], map [sum n] or None) as numpy."""
    N = len(cu_r) - 1
    n_all, m_all = np.diff(cu_r), np.diff(cu_h)
    for what, lens in (("reference", n_all), ("hypothesis", m_all)):
        if N and int(lens.max()) > TEXT_ALIGN_LIMITS["length"]:
            raise ValueError(f"a {what} of {int(lens.max())} symbols: the text alignment kernel takes at most "
                             f"{TEXT_ALIGN_LIMITS['length']} per side")
    if not (_lib.DRY_RUN or (str(device).startswith("cuda") and torch.cuda.is_available())):
        raise _lib.Ta355Error(f"text alignment needs a HIP device (got device={device!r}): there is no CPU path for the tables")
    dev = "cpu" if _lib.DRY_RUN else device
    dist, counts, maps = [], [], []
    step = TEXT_ALIGN_LIMITS["pairs"]
    for a in range(0, N, step):
        b = min(N, a + step)
        to = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)                       # noqa: E731
        cr, ch = cu_r[a:b + 1] - cu_r[a], cu_h[a:b + 1] - cu_h[a]
        d, c, mp, st = torch.ops.ta355.text_align(to(r[cu_r[a]:cu_r[b]]), to(cr), to(h[cu_h[a]:cu_h[b]]), to(ch), int(n_all[a:b].max()),
                                                  int(m_all[a:b].max()), mode, want_path, int(col_block), int(row_block), None)
        st = st.cpu().numpy()
        if not _lib.DRY_RUN and st.any():
            raise _lib.Ta355Error(f"ta_text_align_i32 refused a pair (status {st.tolist()})")
        dist.append(d.cpu().numpy())
        counts.append(c.cpu().numpy())
        if want_path:
            maps.append(mp.cpu().numpy())
    cat = lambda xs, shape: np.concatenate(xs) if xs else np.zeros(shape, np.int32)            # noqa: E731
    return cat(dist, (0,)), cat(counts, (0, 4)), (cat(maps, (0,)) if want_path else None)


def error_counts(refs: Sequence[str], hyps: Sequence[str], unit: str = "word", normalize: Optional[Callable[[str], str]] = None,
                 device="cuda", return_map: bool = False, **tiling) -> dict:
    """Per-pair ``dist``, ``hits``, ``substitutions``, ``deletions``, ``insertions``, ``ref_len``, ``hyp_len`` (int arrays) and the
    corpus rate ``wer`` (``cer`` for ``unit="char"``) = sum(dist) / sum(ref_len), two Python integers divided.  The split of an edit
    distance into S / D / I follows the contract's tie rule (diagonal, then deletion, then insertion).  An empty reference adds its
    hypothesis's length to the edits and nothing to the denominator; only sum(ref_len) == 0 raises.  ``return_map``: also ``map``, per
    pair the hypothesis index matched to every reference position (-1: deleted)."""
    r, cu_r, h, cu_h = encode(refs, hyps, unit, normalize)
    ref_len, hyp_len = np.diff(cu_r).astype(np.int64), np.diff(cu_h).astype(np.int64)
    total = int(ref_len.sum())
    if total == 0:
        raise ValueError("empty reference")
    dist, counts, mp = _device_align(r, cu_r, h, cu_h, TEXT_ALIGN_EDIT, True, device, **tiling)
    out = dict(dist=dist, hits=counts[:, 0], substitutions=counts[:, 1], deletions=counts[:, 2], insertions=counts[:, 3],
               ref_len=ref_len, hyp_len=hyp_len)
    out["cer" if unit == "char" else "wer"] = int(dist.astype(np.int64).sum()) / total
    if return_map:
        out["map"] = [mp[cu_r[p]:cu_r[p + 1]] for p in range(len(ref_len))]
    return out


def align_words_to_reference(pred_words: list, ref_words: list, normalizer, device="cuda") -> list:
    """The reference's LCS-based monotonic matching of predicted words to reference words: a list of (pred_word, ref_word) pairs of
    the input dicts, in chronological order.  ``normalizer.normalize(word)`` is applied to every word; reference words ``<unk>`` and
    words that normalise to nothing are skipped, as there."""
    ref_n = []
    for rw in ref_words:
        word = rw.get("word", "")
        if word == "<unk>":
            continue
        norm = normalizer.normalize(word).strip()
        if norm:
            ref_n.append((norm, rw))
    pred_n = []
    for pw in pred_words:
        norm = normalizer.normalize(pw.get("word", "")).strip()
        if norm:
            pred_n.append((norm, pw))
    if not ref_n or not pred_n:
        return []
    table: dict = {}
    r, cu_r = _ragged([[table.setdefault(w, len(table)) for w, _ in ref_n]])
    h, cu_h = _ragged([[table.setdefault(w, len(table)) for w, _ in pred_n]])
    _, _, mp = _device_align(r, cu_r, h, cu_h, TEXT_ALIGN_LCS, True, device)
    return [(pred_n[int(j)][1], ref_n[i][1]) for i, j in enumerate(mp) if j >= 0]

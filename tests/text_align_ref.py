"""The contract of text alignment (csrc/text_align.hip, tiny_audio_amd/text_align.py) restated in numpy: the truth every test compares
with, by exact integer equality.

Two recurrences over a reference ``r`` (length n) and a hypothesis ``h`` (length m) of int32 symbol ids; only equality is used.

``edit``  D[0][j] = j, D[i][0] = i, D[i][j] = min(D[i-1][j-1] + (r_i != h_j), D[i-1][j] + 1, D[i][j-1] + 1).  The walk from (n, m)
          while i > 0 or j > 0: diagonal if i, j > 0 and D[i][j] == D[i-1][j-1] + (r_i != h_j) (hit if equal, else substitution);
          else deletion (i -= 1) if i > 0 and D[i][j] == D[i-1][j] + 1; else insertion (j -= 1).
``lcs``   L[i][j] = L[i-1][j-1] + 1 if r_i == h_j else max(L[i-1][j], L[i][j-1]).  The walk from (n, m) while i > 0 and j > 0: a pair
          and a diagonal step if r_i == h_j; else i -= 1 if L[i-1][j] > L[i][j-1]; else j -= 1.
          (scripts/eval/evaluators/alignment.py:12-79 of the reference.)

Outputs: ``dist`` = D[n][m] or L[n][m]; ``counts`` = (hits, substitutions, deletions, insertions), in lcs mode (pairs, 0, n - pairs,
m - pairs); ``map`` int32 [n]: the hypothesis index of every reference position's diagonal step, -1 where deleted / unmatched.

Each table has a cell-by-cell form (``*_table_cells``, the definition) and a row-scan form (``*_rows``: a whole row at a time from the
one above, which is what makes a row parallel); tests/test_text_align_host.py holds them equal.  The row-scan form keeps two decision
bits per cell (edit: "the diagonal achieves D", "up achieves D"; lcs: "equal", "up > left"), enough for either walk.
"""
import numpy as np

EDIT, LCS = 0, 1


# ----------------------------------------------------------------------------- the definitions, cell by cell
def edit_table_cells(r, h):
    n, m = len(r), len(h)
    D = [[0] * (m + 1) for _ in range(n + 1)]
    for j in range(m + 1):
        D[0][j] = j
    for i in range(1, n + 1):
        D[i][0] = i
        for j in range(1, m + 1):
            D[i][j] = min(D[i - 1][j - 1] + (r[i - 1] != h[j - 1]), D[i - 1][j] + 1, D[i][j - 1] + 1)
    return D


def lcs_table_cells(r, h):
    n, m = len(r), len(h)
    L = [[0] * (m + 1) for _ in range(n + 1)]
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            L[i][j] = L[i - 1][j - 1] + 1 if r[i - 1] == h[j - 1] else max(L[i - 1][j], L[i][j - 1])
    return L


def edit_walk_cells(D, r, h):
    """-> (counts, map) by the contract's tie rule, from the full table."""
    i, j = len(r), len(h)
    hits = subs = dels = ins = 0
    mp = np.full(len(r), -1, np.int32)
    while i > 0 or j > 0:
        if i > 0 and j > 0 and D[i][j] == D[i - 1][j - 1] + (r[i - 1] != h[j - 1]):
            if r[i - 1] == h[j - 1]:
                hits += 1
            else:
                subs += 1
            mp[i - 1] = j - 1
            i, j = i - 1, j - 1
        elif i > 0 and D[i][j] == D[i - 1][j] + 1:
            dels += 1
            i -= 1
        else:
            ins += 1
            j -= 1
    return (hits, subs, dels, ins), mp


def lcs_walk_cells(L, r, h):
    i, j = len(r), len(h)
    pairs = 0
    mp = np.full(len(r), -1, np.int32)
    while i > 0 and j > 0:
        if r[i - 1] == h[j - 1]:
            mp[i - 1] = j - 1
            pairs += 1
            i, j = i - 1, j - 1
        elif L[i - 1][j] > L[i][j - 1]:
            i -= 1
        else:
            j -= 1
    return (pairs, 0, len(r) - pairs, len(h) - pairs), mp


def align_cells(r, h, mode):
    """(dist, counts, map) straight from the definitions (a Python double loop: small inputs only)."""
    r, h = [int(x) for x in r], [int(x) for x in h]
    if mode == EDIT:
        D = edit_table_cells(r, h)
        counts, mp = edit_walk_cells(D, r, h)
    else:
        D = lcs_table_cells(r, h)
        counts, mp = lcs_walk_cells(D, r, h)
    return D[len(r)][len(h)], counts, mp


# ----------------------------------------------------------------------------- the row scans
def edit_rows(r, h, want_bits=True):
    """Row i from row i - 1 as a scan: A[0] = i, A[j] = min(D[i-1][j] + 1, D[i-1][j-1] + (r_i != h_j)), D[i][j] = j + prefixmin(A[k] - k).
    -> (last row D[n][:], bit0 [n, m] bool "the diagonal achieves D", bit1 [n, m] bool "up achieves D"); the bits None if not wanted."""
    r, h = np.asarray(r, np.int32), np.asarray(h, np.int32)
    n, m = len(r), len(h)
    idx = np.arange(m + 1, dtype=np.int64)
    prev = idx.copy()
    b0 = np.zeros((n, m), bool) if want_bits else None
    b1 = np.zeros((n, m), bool) if want_bits else None
    A = np.empty(m + 1, np.int64)
    for i in range(1, n + 1):
        sub = prev[:-1] + (h != r[i - 1])
        A[0] = i
        np.minimum(prev[1:] + 1, sub, out=A[1:])
        cur = idx + np.minimum.accumulate(A - idx)
        if want_bits:
            b0[i - 1] = cur[1:] == sub
            b1[i - 1] = cur[1:] == prev[1:] + 1
        prev = cur
    return prev, b0, b1


def lcs_rows(r, h, want_bits=True):
    """Row i from row i - 1 as a scan: B[0] = 0, B[j] = max(L[i-1][j], L[i-1][j-1] + eq), L[i][j] = prefixmax(B).
    -> (last row, bit0 "equal", bit1 "up > left")."""
    r, h = np.asarray(r, np.int32), np.asarray(h, np.int32)
    n, m = len(r), len(h)
    prev = np.zeros(m + 1, np.int64)
    b0 = np.zeros((n, m), bool) if want_bits else None
    b1 = np.zeros((n, m), bool) if want_bits else None
    B = np.zeros(m + 1, np.int64)
    for i in range(1, n + 1):
        eq = h == r[i - 1]
        np.maximum(prev[1:], prev[:-1] + eq, out=B[1:])
        cur = np.maximum.accumulate(B)
        if want_bits:
            b0[i - 1] = eq
            b1[i - 1] = prev[1:] > cur[:-1]
        prev = cur
    return prev, b0, b1


def walk_bits(n, m, b0, b1, mode, dist):
    """Either walk on the two decision bits alone -> (counts, map).  Substitutions follow from dist = S + D + I."""
    i, j = n, m
    diag = dels = ins = 0
    mp = np.full(n, -1, np.int32)
    while i > 0 and j > 0:
        if b0[i - 1, j - 1]:
            mp[i - 1] = j - 1
            diag += 1
            i, j = i - 1, j - 1
        elif b1[i - 1, j - 1]:
            dels += 1
            i -= 1
        else:
            ins += 1
            j -= 1
    if mode == LCS:
        return (diag, 0, n - diag, m - diag), mp
    dels, ins = dels + i, ins + j
    subs = dist - dels - ins
    return (diag - subs, subs, dels, ins), mp


def align(r, h, mode, want_path=True):
    """(dist, counts, map) by the row scan; counts and map None without ``want_path``."""
    rows = edit_rows if mode == EDIT else lcs_rows
    last, b0, b1 = rows(r, h, want_bits=want_path)
    dist = int(last[-1])
    if not want_path:
        return dist, None, None
    counts, mp = walk_bits(len(r), len(h), b0, b1, mode, dist)
    return dist, counts, mp


def align_batch(refs, hyps, mode, want_path=True):
    """Lists of id arrays -> (dist int32 [N], counts int32 [N, 4], map int32 [sum n]) as the device lays them out."""
    N = len(refs)
    dist = np.zeros(N, np.int32)
    counts = np.zeros((N, 4), np.int32)
    maps = []
    for p, (r, h) in enumerate(zip(refs, hyps)):
        d, c, mp = align(r, h, mode, want_path)
        dist[p] = d
        if want_path:
            counts[p] = c
            maps.append(mp)
    return dist, counts, (np.concatenate(maps) if maps else np.zeros(0, np.int32)).astype(np.int32)


def ragged(seqs):
    """Lists of id arrays -> (flat int32, cu int32 [N + 1])."""
    cu = np.zeros(len(seqs) + 1, np.int32)
    cu[1:] = np.cumsum([len(s) for s in seqs])
    flat = np.concatenate([np.asarray(s, np.int32) for s in seqs]) if len(seqs) and cu[-1] else np.zeros(0, np.int32)
    return flat.astype(np.int32), cu

"""The definition of forced alignment that csrc/align.hip is held to: the recurrence and the walk of the reference's
``ForcedAligner._get_trellis`` / ``_backtrack`` (tiny_audio/alignment.py:47-152) restated as literal loops in numpy float32.

Test infrastructure (like tests/attention_ref.py): slow, obvious, and equal to the reference bit for bit, which
tests/test_alignment_host.py checks against tests/golden/alignment.npz (written by the reference itself).
"""
import numpy as np

F32 = np.float32
NEG = F32(-np.inf)


def trellis(emission, tokens, blank_id=0):
    """emission f32 [T, C], tokens ints -> (trellis f32 [T + 1, J + 1], move bool [T + 1, J + 1]).  ``move[t + 1, j]`` is the
    decision "move >= stay" of cell (t + 1, j): what the backtrack compares when it stands there."""
    e = np.asarray(emission, F32)
    T, J = e.shape[0], len(tokens)
    tr = np.full((T + 1, J + 1), NEG, F32)
    mv = np.zeros((T + 1, J + 1), bool)
    tr[0, 0] = 0
    with np.errstate(invalid="ignore"):
        for t in range(T):
            eb = e[t, blank_id]
            for j in range(J + 1):
                stay = F32(tr[t, j] + eb)
                move = F32(tr[t, j - 1] + e[t, tokens[j - 1]]) if j > 0 else NEG
                tr[t + 1, j] = move if move > stay else stay          # Python's max(stay, move)
                mv[t + 1, j] = j > 0 and move >= stay
    return tr, mv


def trellis_fast(emission, tokens, blank_id=0):
    """The same values with the token loop vectorised (each cell is still one f32 add per candidate and one comparison), for the
    shapes at which the literal loop is too slow for a test."""
    e = np.asarray(emission, F32)
    T, J = e.shape[0], len(tokens)
    tok = np.asarray(tokens, np.int64).reshape(-1)
    tr = np.full((T + 1, J + 1), NEG, F32)
    mv = np.zeros((T + 1, J + 1), bool)
    tr[0, 0] = 0
    with np.errstate(invalid="ignore"):
        for t in range(T):
            stay = tr[t] + e[t, blank_id]
            move = np.full(J + 1, NEG, F32)
            move[1:] = tr[t, :-1] + e[t, tok]
            tr[t + 1] = np.where(move > stay, move, stay)
            mv[t + 1, 1:] = move[1:] >= stay[1:]
    return tr, mv


def backtrack(tr, mv, tokens):
    """-> (status, frames): status 1 and no frames when trellis[T, J] is -inf (the reference then falls back to uniform spans),
    else status 0 and the frame of every token: from (T, J), while t > 0 and j > 0, a move puts token j - 1 on frame t - 1."""
    T, J = tr.shape[0] - 1, tr.shape[1] - 1
    if J == 0:
        return 0, []
    if tr[T, J] == NEG:
        return 1, []
    frames = [-1] * J
    t, j = T, J
    while t > 0 and j > 0:
        if mv[t, j]:
            frames[j - 1] = t - 1
            j -= 1
        t -= 1
    assert j == 0, "a finite trellis[T, J] is reached through J moves"
    return 0, frames


def spans(tokens, status, frames, num_frames):
    """The reference's return value of ``_backtrack``: (token, start_frame, end_frame) per token, Python floats."""
    J = len(tokens)
    if J == 0:
        return []
    if status:
        per = num_frames / J
        return [(tokens[i], i * per, (i + 1) * per) for i in range(J)]
    return [(tokens[i], float(frames[i]), float(frames[i]) + 1.0) for i in range(J)]


def align(emission, tokens, blank_id=0, fast=False):
    """-> dict(trellis, status, frames, score)."""
    tr, mv = (trellis_fast if fast else trellis)(emission, tokens, blank_id)
    status, frames = backtrack(tr, mv, tokens)
    return dict(trellis=tr, status=status, frames=frames, score=tr[-1, -1])

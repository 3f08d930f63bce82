"""Numpy restatements of csrc/segment.hip (the contract of include/ta355.h, "long-form segmentation").

* ``cut_cost``      the cost of cutting at every position, in float64 (the yardstick of the f32 kernel's error bound);
* ``cut_plan``      the dynamic programme in float32, operation by operation, with the tie rule (lowest predecessor);
* ``plan_by_enumeration``  every cut set of a small grid, for tests/test_segment_ref.py;
* ``gather``        the padded window batch.
"""
import itertools

import numpy as np

HOP, POWER_WINDOW = 160, 400
U = 2.0 ** -24


def positions(n: int) -> int:
    """T: the grid of a recording of n samples is p = 0 .. T."""
    return -(-int(n) // HOP)


def cost_K(h: int) -> int:
    """TA_CUT_COST_K(h) of include/ta355.h."""
    return max(2 * h + 25, 65)


def gamma(K: int) -> float:
    return K * U / (1.0 - K * U)


def cut_cost(x, h: int = 10, cut_penalty: float = 0.05) -> np.ndarray:
    """float64 [T + 1]: s[p] + cut_penalty * mean power, cut_penalty as the float32 the kernel receives."""
    x = np.asarray(x, np.float32).astype(np.float64)
    n = x.shape[0]
    T = positions(n)
    half = POWER_WINDOW // 2
    sq = np.zeros(half + HOP * T + half, np.float64)
    sq[half:half + n] = x * x
    pw = np.array([sq[HOP * p:HOP * p + POWER_WINDOW].sum() for p in range(T + 1)]) / POWER_WINDOW
    pad = np.zeros(T + 1 + 2 * h, np.float64)
    pad[h:h + T + 1] = pw
    s = np.array([pad[p:p + 2 * h + 1].sum() for p in range(T + 1)]) / (2 * h + 1)
    return s + float(np.float32(cut_penalty)) * (sq.sum() / n)


def cut_plan(cost, T: int, min_len: int, max_len: int):
    """-> (cuts list, n_seg, dp_T float32, back int32 [T + 1], dp float32 [T + 1]) as ta_cut_plan_f32 defines them."""
    cost = np.asarray(cost, np.float32)
    dp = np.full(T + 1, np.inf, np.float32)
    back = np.full(T + 1, -1, np.int32)
    dp[0] = 0.0
    for p in range(1, T + 1):
        lo, hi = max(0, p - max_len), p - min_len
        if hi < 0:
            continue
        w = dp[lo:hi + 1]
        k = int(np.argmin(w))                      # the first, hence lowest, position of the minimum
        back[p] = lo + k
        dp[p] = np.float32(cost[p] if p < T else 0.0) + w[k]
    if T < min_len:
        return [0, T], 1, np.float32(0.0), back, dp
    cuts, p = [T], T
    while p > 0:
        p = int(back[p])
        assert p >= 0
        cuts.append(p)
    return cuts[::-1], len(cuts) - 1, dp[T], back, dp


def plan_by_enumeration(cost, T: int, min_len: int, max_len: int):
    """Every set of interior cuts with all windows within [min_len, max_len] -> (the least total cost, every cut list attaining it).
    Sums in float64: the tests use costs k / 64, whose sums are exact in both widths."""
    best, argbest = None, []
    for k in range(0, T):
        for inner in itertools.combinations(range(1, T), k):
            cuts = [0, *inner, T]
            if any(not min_len <= b - a <= max_len for a, b in zip(cuts[:-1], cuts[1:])):
                continue
            total = float(sum(float(cost[c]) for c in inner))
            if best is None or total < best:
                best, argbest = total, [cuts]
            elif total == best:
                argbest.append(cuts)
    return best, argbest


def gather(flat, start, length, Ls: int):
    """-> (float32 [W, Ls], int64 [W])."""
    flat = np.asarray(flat, np.float32)
    out = np.zeros((len(start), Ls), np.float32)
    lens = np.zeros(len(start), np.int64)
    for w, (s, n) in enumerate(zip(start, length)):
        n = min(max(int(n), 0), Ls)
        out[w, :n] = flat[int(s):int(s) + n]
        lens[w] = n
    return out, lens

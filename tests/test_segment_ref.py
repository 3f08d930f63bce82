"""-m "not gpu": the recurrence of ta_cut_plan_f32 (tests/segment_ref.py, which the device is held to bit for bit) against exhaustive
enumeration of every cut set: feasible, optimal, and the tie rule -- ``back[p]`` is the LOWEST predecessor that attains the minimum,
so the walk from T picks the lowest last cut among the optimal plans, then the lowest one before it, and so on.  Costs are k / 64:
their float32 sums are exact, so "optimal" is an equality."""
import numpy as np
import pytest

from tests import segment_ref as R


def _cases():
    rng = np.random.RandomState(5)
    out = []
    for min_len in (1, 2, 3):
        for extra in range(4):
            for T in range(min_len, 15):
                out.append((T, min_len, 2 * min_len + extra, rng.randint(0, 64, size=T + 1) / 64.0))
    return out


def _check(T, min_len, max_len, cost):
    cuts, n_seg, dp_T, back, dp = R.cut_plan(cost, T, min_len, max_len)
    best, argbest = R.plan_by_enumeration(cost, T, min_len, max_len)
    assert best is not None, "2 * min_len <= max_len: a plan exists for every T >= min_len"
    assert cuts[0] == 0 and cuts[-1] == T and n_seg == len(cuts) - 1
    assert all(min_len <= b - a <= max_len for a, b in zip(cuts[:-1], cuts[1:]))
    assert float(dp_T) == best == sum(float(cost[c]) for c in cuts[1:-1])
    assert cuts == min(argbest, key=lambda c: c[::-1])
    for p in range(1, T + 1):                      # every entry, not only those on the walk
        lo, hi = max(0, p - max_len), p - min_len
        if hi < 0:
            assert back[p] == -1 and np.isinf(dp[p])
        else:
            w = dp[lo:hi + 1]
            assert back[p] == lo + int(np.flatnonzero(w == w.min())[0])


def test_plan_is_feasible_optimal_and_breaks_ties_low():
    cases = _cases()
    assert len(cases) > 130
    for T, min_len, max_len, cost in cases:
        _check(T, min_len, max_len, cost)


@pytest.mark.parametrize("min_len,max_len", [(1, 2), (2, 5), (3, 6), (3, 9)])
def test_all_equal_costs(min_len, max_len):
    """Every plan with the fewest cuts ties: the rule decides alone."""
    for T in range(min_len, 15):
        _check(T, min_len, max_len, np.full(T + 1, 0.25))
        cuts = R.cut_plan(np.full(T + 1, 0.25), T, min_len, max_len)[0]
        assert len(cuts) - 1 == -(-T // max_len)


def test_shorter_than_the_minimum_is_one_window():
    for T, min_len in ((1, 2), (2, 3), (1, 3)):
        cuts, n_seg, dp_T, back, dp = R.cut_plan(np.ones(T + 1), T, min_len, 2 * min_len)
        assert cuts == [0, T] and n_seg == 1 and dp_T == 0.0
        assert (back == -1).all() and np.isinf(dp[1:]).all()


def test_cost_restatement_on_a_hand_case():
    """n = 161: T = 2; position 1 sees samples [-40, 360) of which [0, 161) exist."""
    x = np.arange(1, 162, dtype=np.float32) / 64
    c = R.cut_cost(x, h=0, cut_penalty=0.0)
    sq = x.astype(np.float64) ** 2
    assert c.shape == (3,)
    assert np.isclose(c[0], sq[:200].sum() / 400) and np.isclose(c[1], sq.sum() / 400) and np.isclose(c[2], sq[120:].sum() / 400)
    c2 = R.cut_cost(x, h=1, cut_penalty=0.5)
    assert np.isclose(c2[0], (c[0] + c[1]) / 3 + 0.5 * sq.mean()) and np.isclose(c2[1], c.sum() / 3 + 0.5 * sq.mean())


def test_gather_restatement():
    flat = np.arange(20, dtype=np.float32)
    out, lens = R.gather(flat, [3, 0, 19], [4, 6, 1], 5)
    assert out.tolist() == [[3, 4, 5, 6, 0], [0, 1, 2, 3, 4], [19, 0, 0, 0, 0]] and lens.tolist() == [4, 5, 1]

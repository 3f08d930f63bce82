"""The fp64 reference of the decoding scores (tests/scores_ref.py) against closed forms and torch.log_softmax in float64 (no GPU):
the GPU tests gate the kernel on this reference, so it is pinned here first."""
import numpy as np
import torch

from tests.scores_ref import token_scores_ref


def test_uniform_row_has_closed_form():
    for V in (1, 2, 65, 4099):
        x = np.full((2, V + 3), 1.25, np.float32)
        x[:, V:] = np.nan                                      # columns >= V must not matter
        lp, ent, ids, tl = token_scores_ref(x, V, np.array([0, V - 1]), min(V, 4))
        np.testing.assert_allclose(lp, -np.log(V), rtol=0, atol=1e-13)
        np.testing.assert_allclose(ent, np.log(V), rtol=0, atol=1e-12)
        assert ids[0].tolist() == list(range(min(V, 4)))       # all tied: index order
        np.testing.assert_allclose(tl, -np.log(V), rtol=0, atol=1e-13)


def test_single_survivor():
    x = np.full((1, 40), -np.inf, np.float32)
    x[0, 17] = -3.5
    lp, ent, ids, tl = token_scores_ref(x, 40, np.array([17]), 4)
    assert lp[0] == 0.0 and ent[0] == 0.0
    assert ids[0].tolist() == [17, -1, -1, -1] and tl[0, 0] == 0.0 and np.isneginf(tl[0, 1:]).all()
    lp, _, _, _ = token_scores_ref(x, 40, np.array([3]), 0)    # a chosen -inf entry: -inf, not NaN
    assert np.isneginf(lp[0])
    _, _, ids0, tl0 = token_scores_ref(x, 40, np.array([17]), 0)
    assert ids0.shape == (1, 0) and tl0.shape == (1, 0)


def test_against_log_softmax_float64():
    rng = np.random.RandomState(0)
    V = 301
    x = (4.0 * rng.standard_normal((5, V + 5))).astype(np.float32)
    x[1, rng.choice(V, 250, replace=False)] = -np.inf
    x[2, :V] += 3e4
    x[3, :V] -= 3e4
    chosen = np.array([int(np.argmax(x[b, :V])) for b in range(5)])
    chosen[4] = int(np.argmin(x[4, :V]))
    lp, ent, ids, tl = token_scores_ref(x, V, chosen, V)       # k = V: every entry
    ls = torch.log_softmax(torch.from_numpy(x[:, :V].astype(np.float64)), dim=-1)
    p = ls.exp()
    want_ent = -(torch.where(p > 0, p * ls, torch.zeros_like(p))).sum(-1).numpy()
    np.testing.assert_allclose(lp, ls.numpy()[np.arange(5), chosen], rtol=0, atol=1e-11)
    np.testing.assert_allclose(ent, want_ent, rtol=0, atol=1e-11)
    for b in range(5):
        n = int(np.isfinite(x[b, :V]).sum())
        assert (ids[b, n:] == -1).all() and np.isneginf(tl[b, n:]).all()
        np.testing.assert_allclose(tl[b, :n], ls.numpy()[b, ids[b, :n]], rtol=0, atol=1e-11)
        assert (np.diff(tl[b, :n]) <= 0).all()
        assert abs(np.log(np.exp(tl[b, :n]).sum())) < 1e-12   # logsumexp of all the alternatives is 0
        assert ids[b, 0] == np.argmax(x[b, :V])


def test_ties_are_ordered_by_index():
    x = np.zeros((1, 64), np.float32)
    x[0, [50, 7, 23]] = 2.0                                    # three exact duplicates of the maximum
    x[0, 40] = 1.0
    _, _, ids, tl = token_scores_ref(x, 64, np.array([7]), 6)
    assert ids[0].tolist() == [7, 23, 50, 40, 0, 1]
    assert tl[0, 0] == tl[0, 1] == tl[0, 2] > tl[0, 3] > tl[0, 4] == tl[0, 5]

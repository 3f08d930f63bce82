"""tests/beam_ref.py against HF's own beam search (tests/golden/beam_search.npz, written by tests/golden/make_beam_fixture.py from the
installed transformers on the CPU): fed HF's per-step processed rows, the restatement must return HF's sequences and sequence scores
EXACTLY, for every run of the fixture (K in {1, 2, 4}, three length penalties, three early-stopping modes, 0 / 1 / 2 eos ids,
num_return_sequences 1 and K, one run through repetition_penalty and min_new_tokens).  No GPU."""
import json
import os

import numpy as np
import pytest

from tests import beam_ref as BR

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "beam_search.npz")
G = np.load(PATH)
META = json.loads(str(G["meta"]))


def _rows(i, V):
    tv, ti = G[f"r{i}_top_val"], G[f"r{i}_top_idx"].astype(np.int64)
    rows = np.full(tv.shape[:2] + (V,), -np.inf, np.float32)
    np.put_along_axis(rows, ti, tv, -1)
    return rows


@pytest.mark.parametrize("i", range(len(META["runs"])))
def test_restatement_returns_hfs_sequences_and_scores(i):
    run, V, B, max_new = META["runs"][i], META["V"], META["B"], META["max_new"]
    st = BR.run_rows(_rows(i, V), B, run["K"], max_new, V, eos_ids=run["eos"], pad_id=META["pad"], length_penalty=run["length_penalty"],
                     early_stopping=run["early_stopping"])
    n = run["num_return_sequences"]
    assert st.pool_fin[:, :n].all()                                         # every returned slot is a finished hypothesis
    seq, score = st.result(n)
    assert np.array_equal(seq, G[f"r{i}_sequences"]), (seq, G[f"r{i}_sequences"])
    if run["K"] > 1:                                                        # (K = 1 is HF's greedy search: tokens only)
        assert score.dtype == np.float32 and np.array_equal(score, G[f"r{i}_sequences_scores"])
    lens = (G[f"r{i}_beam_indices"] >= 0).sum(-1)                            # HF's own length of every returned hypothesis
    assert np.array_equal(st.pool_len[:, :n].reshape(-1), lens)


def test_fixture_covers_what_it_claims():
    runs = META["runs"]
    assert {r["K"] for r in runs} == {1, 2, 4} and {r["length_penalty"] for r in runs} == {0.0, 1.0, 2.0}
    assert {str(r["early_stopping"]) for r in runs} == {"False", "True", "never"} and {len(r["eos"]) for r in runs} == {0, 1, 2}
    assert any(r["num_return_sequences"] == r["K"] > 1 for r in runs) and any(r["extra"] for r in runs)
    # some hypotheses finish early and others run to the maximum length
    lens = np.concatenate([(G[f"r{i}_beam_indices"] >= 0).sum(-1) for i in range(len(runs))])
    assert lens.min() < META["max_new"] and lens.max() == META["max_new"]


def test_stable_topk_and_divisors():
    acc = np.array([[1.0, 3.0, 3.0, -np.inf, 2.0, -np.inf]], np.float32)
    v, i = BR.topk_stable(acc, 6)
    assert i.tolist() == [[1, 2, 4, 0, 3, 5]] and v[0, 0] == 3.0
    assert BR.length_divisors(0.0, 3).tolist() == [1.0, 1.0, 1.0] and BR.length_divisors(2.0, 3).tolist() == [1.0, 4.0, 9.0]
    assert BR.n_candidates(4, 0) == 8 and BR.n_candidates(4, 1) == 8 and BR.n_candidates(4, 3) == 16

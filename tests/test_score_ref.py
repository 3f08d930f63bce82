"""Pins tests/score_ref.py (the candidate-scoring reference) on the generate_small.npz model, without a GPU: against the step-by-step
teacher-forced logits of tests/scores_ref.py, and against the identities any probability distribution over token sequences obeys.

Bounds: both sides of the first test are the same fp32 oracle run over different batch shapes (one pass over prompt + 12 tokens against
12 growing passes), so they differ by fp32 matmul rounding only: a logit of magnitude <= 64 carries at most a few 1e-5 of it, gated at
2e-4 per token.  The identities hold in float64 given one fp32 logits row: sum_v exp(lp_v) - 1 is rounding of 1024 float64 terms
(gated at 1e-9); the two-token marginal sums 1024 products exp(lp_0 + lp_1) whose first factor comes from 1024 rows of one fp32 pass and
is compared with a pass of one row, so it inherits the 2e-4 of the first test, relative to exp(score(c_0)).
"""
import numpy as np
import pytest

from oracle import weights as OW
from tests import score_ref as SR
from tests.golden import recipe as R
from tests.scores_ref import teacher_forced_logits


@pytest.fixture(scope="module")
def ctx(golden):
    g = golden("generate_small.npz")
    S = R.SMALL
    E, D, H = S["enc"]["hidden"], S["lm"]["hidden"], S["proj_hidden"]
    W = dict(encoder=OW.init_encoder(S["enc"], 0), lm=R.gen_lm_weights(), projector=OW.init_mlp_projector(E, D, H))
    cfg = dict(enc=S["enc"], lm=S["lm"], projector_type="mlp", k=S["k"], audio_token_id=S["audio_token_id"])
    batch = dict(input_ids=g["input_ids"], input_features=g["input_features"])
    return dict(W=W, cfg=cfg, batch=batch, x=SR.prompt_rows(batch, W, cfg), tokens=np.asarray(g["tokens_a"], np.int64), V=S["lm"]["vocab"])


def test_greedy_tokens_score_is_the_teacher_forced_sum(ctx):
    tokens = ctx["tokens"]
    steps, _ = teacher_forced_logits(ctx["batch"], ctx["W"], ctx["cfg"], tokens)
    lp = SR.token_logprobs(ctx["x"], ctx["W"], ctx["cfg"], [[tokens[0].tolist()], [tokens[1].tolist()]])
    sc = SR.scores(ctx["x"], ctx["W"], ctx["cfg"], [[tokens[0].tolist()], [tokens[1].tolist()]])
    for b in range(2):
        want = np.array([SR.log_softmax64(steps[t][b, :ctx["V"]])[tokens[b, t]] for t in range(tokens.shape[1])])
        d = float(np.abs(lp[b][0] - want).max())
        print(f"clip {b}: max |score_ref lp_t - teacher-forced lp_t| = {d:.2e}")
        assert lp[b][0].shape == want.shape and d <= 2e-4
        assert abs(sc[b][0] - float(np.sum(lp[b][0]))) <= 1e-12 * max(1.0, abs(sc[b][0]))


def test_one_token_candidates_sum_to_one(ctx):
    sc = SR.scores(ctx["x"], ctx["W"], ctx["cfg"], [[[v] for v in range(ctx["V"])], []])
    assert sc[1] == [] and len(sc[0]) == ctx["V"]
    assert abs(float(np.exp(np.asarray(sc[0])).sum()) - 1.0) <= 1e-9


def test_two_token_marginal(ctx):
    c0 = int(ctx["tokens"][1, 0])
    one = SR.scores(ctx["x"], ctx["W"], ctx["cfg"], [[], [[c0]]])[1][0]
    two = SR.scores(ctx["x"], ctx["W"], ctx["cfg"], [[], [[c0, v] for v in range(ctx["V"])]])[1]
    total = float(np.exp(np.asarray(two)).sum())
    print(f"two-token marginal: relative gap {abs(total - np.exp(one)) / np.exp(one):.2e}")
    assert abs(total - np.exp(one)) <= 2e-4 * np.exp(one)
